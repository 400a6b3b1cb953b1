// skh_variance.h -- variance guidance (skh_moments, skh_denoise_variance; include/strelka_hip.h and DESIGN.md section 2 "Variance guidance" are the definition).
//
//   k_vr_moments    one lane, one pixel: the luminance of the raw colour, its first two moments blended with the previous frame's through the taps skh_temporal
//                   accepted (the mask word of its motion plane), the variance.  The projection is k_tp_reproject's, restated: that kernel is left as it is.
//   k_vr_pack       k_dn_pack with the variance in the colour record's fourth word: {rgb or demodulated rgb, v0}, v0 >= 0 on a surface pixel and -1 on every
//                   other.  The guide record is k_dn_pack's, so a tap of the level kernel stays at 40 bytes.
//   k_vr_estimate   launched only with SKH_VDENOISE_ESTIMATE, from k_vr_pack's colour image into the second one: a surface pixel whose moments are younger than
//                   min_history replaces v0 by the 7 x 7 estimate; every other record is copied.  (A pass of its own, into an image of its own: it reads its
//                   neighbours' records, so it must not write where it reads.)  The branch is taken by whole waves where a region was disoccluded.
//   k_vr_level      k_dn_level with the luminance stop 1 / (sigma sqrt(vbar) + epsilon) in place of the colour stop, and the variance filtered with the squared
//                   weights.  The last launch writes the caller's image and, when given, the moments record with the filtered variance.
//
// Workgroups, the one-dimensional grid, the clamped addresses and the selection of skipped taps are k_dn_level's.  No LDS, no atomics, no scratch.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_denoise.h"
#include "skh_temporal.h"

namespace skh
{

struct VrP // by-value kernel argument of the three filter kernels
{
    uint32_t width, height;
    uint32_t step;          // 1 << level
    float sigmaLuminance;   // finite, or lumOff
    float epsilon, kn, kp;  // kn, kp as DnP's
    float albedoFloor, minHistory;
    uint32_t flags;         // k_vr_pack: SKH_DENOISE_DEMODULATE; k_vr_level<true>: SKH_DENOISE_REMODULATE
    uint32_t lumOff;        // sigma_luminance == +inf: the luminance term is 0, not inf * 0
};

SKH_DI float vr_lum(float r, float g, float b)
{
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}
// the normal and the plane term of skh_denoise for the tap (gq, pq) seen from the centre (gp, pp): {N.xyz, P.x}, {P.y, P.z}
SKH_DI void vr_guides(const float4& gp, const float2& pp, const float4& gq, const float2& pq, float kn, float kp, float& tn, float& tp)
{
    const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
    tn = ((nx * nx + ny * ny) + nz * nz) * kn;
    const float px = gq.w - gp.w, py = pq.x - pp.x, pz = pq.y - pp.y;
    const float d = (gp.x * px + gp.y * py) + gp.z * pz;
    tp = (d * d) * kp;
}
// a packed colour record belongs to a surface pixel unless its fourth word is negative
SKH_DI bool vr_surface(float w)
{
    return !(w < 0.0f);
}

// ---- skh_moments ----
__global__ void __launch_bounds__(256) k_vr_moments(TpP tp, const float4* __restrict__ color, const uint4* __restrict__ ids, const float4* __restrict__ position,
                                                     const float4* __restrict__ albedo, const float4* __restrict__ motion,
                                                     const float4* __restrict__ prevMoments, float4* __restrict__ momentsOut)
{
    const uint32_t tilesX = (tp.width + 63u) / 64u, tileY = blockIdx.x / tilesX;
    const uint32_t x = (blockIdx.x - tileY * tilesX) * 64u + threadIdx.x, y = tileY * 4u + threadIdx.y;
    if (x >= tp.width || y >= tp.height)
        return;
    const uint32_t i = y * tp.width + x;
    const float4 c = color[i];
    const uint32_t kind = ids[i].w;
    if (!((kind == 1u || kind == 2u) && dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z))) // not a surface pixel
    {
        momentsOut[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float cx = c.x, cy = c.y, cz = c.z;
    if (tp.flags & SKH_TEMPORAL_DEMODULATE)
    {
        const float4 a = albedo[i];
        cx = c.x / dn_floor(a.x, tp.albedoFloor), cy = c.y / dn_floor(a.y, tp.albedoFloor), cz = c.z / dn_floor(a.z, tp.albedoFloor);
    }
    const float l = vr_lum(cx, cy, cz), ll = l * l;
    float m1 = l, m2 = ll, nn = tp.initialLength; // the pixel without history
    if (tp.hasPrev)
    {
        const float4 P = position[i];
        const float mw = motion[i].w;
        const uint32_t mask = (mw >= 0.0f && mw <= 15.0f) ? (uint32_t)mw : 0u; // (a NaN gives 0)
        // k_tp_reproject's lines
        const float W = (float)tp.width, H = (float)tp.height;
        const v4 clip = mul44(tp.prevWorldToClip, mk4(P.x, P.y, P.z, 1.0f));
        const float fx = ((clip.x / clip.w) * 0.5f + 0.5f) * W - 0.5f;
        const float fy = ((clip.y / clip.w) * 0.5f + 0.5f) * H - 0.5f;
        const bool projects = clip.w > 0.0f && dn_finite(fx) && dn_finite(fy) && fx >= -1.0f && fx <= W && fy >= -1.0f && fy <= H;
        const float gx = projects ? fx : (float)x, gy = projects ? fy : (float)y;
        const float flx = floorf(gx), fly = floorf(gy);
        const int qx0 = (int)flx, qy0 = (int)fly; // -1 .. W, -1 .. H
        const float tx = gx - flx, ty = gy - fly;
        const float ux = 1.0f - tx, uy = 1.0f - ty;
        const float w[4] = { ux * uy, tx * uy, ux * ty, tx * ty };
        const int Wi = (int)tp.width, Hi = (int)tp.height;
        float4 mq[4];
        bool in[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const int qx = qx0 + (k & 1), qy = qy0 + (k >> 1);
            in[k] = qx >= 0 && qx < Wi && qy >= 0 && qy < Hi;
            const int ax = qx < 0 ? 0 : (qx < Wi ? qx : Wi - 1), ay = qy < 0 ? 0 : (qy < Hi ? qy : Hi - 1);
            mq[k] = prevMoments[(uint32_t)ay * tp.width + (uint32_t)ax];
        }
        float sw = 0.0f, s1 = 0.0f, s2 = 0.0f, sn = 0.0f;
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const bool used = projects && ((mask >> k) & 1u) != 0u && in[k] && w[k] > 0.0f && dn_finite(mq[k].x) && dn_finite(mq[k].y) && dn_finite(mq[k].w) &&
                              mq[k].w >= 1.0f;
            // selected, never multiplied by zero
            sw = used ? sw + w[k] : sw;
            s1 = used ? s1 + w[k] * mq[k].x : s1;
            s2 = used ? s2 + w[k] * mq[k].y : s2;
            sn = used ? sn + w[k] * mq[k].w : sn;
            any = any || used;
        }
        const float h1 = s1 / sw, h2 = s2 / sw, nh = sn / sw;
        const float n1 = nh + 1.0f;
        const float nb = n1 < tp.maxHistory ? n1 : tp.maxHistory;
        const float alpha = 1.0f / nb;
        m1 = any ? h1 + (l - h1) * alpha : l;
        m2 = any ? h2 + (ll - h2) * alpha : ll;
        nn = any ? nb : tp.initialLength;
    }
    const float v = m2 - m1 * m1;
    momentsOut[i] = make_float4(m1, m2, v > 0.0f ? v : 0.0f, nn);
}

// ---- skh_denoise_variance ----
__global__ void __launch_bounds__(256) k_vr_pack(VrP vp, const float4* __restrict__ color, const uint4* __restrict__ ids, const float4* __restrict__ normal,
                                                  const float4* __restrict__ position, const float4* __restrict__ albedo, const float4* __restrict__ moments,
                                                  float4* __restrict__ c0, float4* __restrict__ g0, float2* __restrict__ g1)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= vp.width * vp.height)
        return;
    const float4 c = color[i];
    const uint32_t kind = ids[i].w;
    const bool surface = (kind == 1u || kind == 2u) && dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z);
    float4 rc = make_float4(0.0f, 0.0f, 0.0f, -1.0f), rg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 rp = make_float2(0.0f, 0.0f);
    if (surface)
    {
        const float z = moments[i].z;
        rc = make_float4(c.x, c.y, c.z, (dn_finite(z) && z > 0.0f) ? z : 0.0f);
        if (vp.flags & SKH_DENOISE_DEMODULATE)
        {
            const float4 a = albedo[i];
            rc.x = c.x / dn_floor(a.x, vp.albedoFloor), rc.y = c.y / dn_floor(a.y, vp.albedoFloor), rc.z = c.z / dn_floor(a.z, vp.albedoFloor);
        }
        const float4 n = normal[i], p = position[i];
        rg = make_float4(n.x, n.y, n.z, p.x);
        rp = make_float2(p.y, p.z);
    }
    c0[i] = rc;
    g0[i] = rg;
    g1[i] = rp;
}

__global__ void __launch_bounds__(256) k_vr_estimate(VrP vp, const float4* __restrict__ cin, const float4* __restrict__ g0, const float2* __restrict__ g1,
                                                      const float4* __restrict__ moments, float4* __restrict__ cout)
{
    const uint32_t tilesX = (vp.width + 63u) / 64u, ty = blockIdx.x / tilesX;
    const uint32_t x = (blockIdx.x - ty * tilesX) * 64u + threadIdx.x, y = ty * 4u + threadIdx.y;
    if (x >= vp.width || y >= vp.height)
        return;
    const uint32_t i = y * vp.width + x;
    float4 cp = cin[i];
    if (vr_surface(cp.w))
    {
        const float nm = moments[i].w;
        if (!(nm >= vp.minHistory)) // (a NaN too)
        {
            const float4 gp = g0[i];
            const float2 pp = g1[i];
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            bool any = false;
            const int W = (int)vp.width, H = (int)vp.height;
#pragma unroll 1
            for (int dy = -3; dy <= 3; ++dy)
            {
                const int qy = (int)y + dy;
                const bool rowIn = qy >= 0 && qy < H;
                const uint32_t row = (uint32_t)(rowIn ? qy : (int)y) * vp.width;
#pragma unroll
                for (int dx = -3; dx <= 3; ++dx)
                {
                    const int qx = (int)x + dx;
                    const bool in = rowIn && qx >= 0 && qx < W;
                    const uint32_t j = row + (uint32_t)(in ? qx : (int)x);
                    const float cw = cin[j].w;
                    const float4 mq = moments[j];
                    float tn, tp;
                    vr_guides(gp, pp, g0[j], g1[j], vp.kn, vp.kp, tn, tp);
                    float a = tn + tp;
                    a = a <= 64.0f ? a : 64.0f; // (a NaN too)
                    const float w = skm::expf_(-a);
                    if (in && vr_surface(cw) && dn_finite(mq.x) && dn_finite(mq.y)) // selected, never multiplied by zero
                    {
                        s0 = s0 + w;
                        s1 = s1 + w * mq.x;
                        s2 = s2 + w * mq.y;
                        any = true;
                    }
                }
            }
            const float e1 = s1 / s0, e2 = s2 / s0;
            float v = e2 - e1 * e1;
            v = v > 0.0f ? v : 0.0f;
            const float k = vp.minHistory / (nm >= 1.0f ? nm : 1.0f);
            cp.w = any ? v * k : 0.0f;
        }
    }
    cout[i] = cp;
}

// LAST: this launch writes the caller's image (uint4 words: the pixels it passes through are bit copies) and, when given, the moments record
template <bool LAST>
__global__ void __launch_bounds__(256) k_vr_level(VrP vp, const float4* __restrict__ cin, const float4* __restrict__ g0, const float2* __restrict__ g1,
                                                   float4* __restrict__ cout, const uint4* color, const float4* __restrict__ albedo, uint4* out,
                                                   const float4* moments, float4* momentsOut)
{
    const uint32_t tilesX = (vp.width + 63u) / 64u, ty = blockIdx.x / tilesX;
    const uint32_t x = (blockIdx.x - ty * tilesX) * 64u + threadIdx.x, y = ty * 4u + threadIdx.y;
    if (x >= vp.width || y >= vp.height)
        return;
    const uint32_t i = y * vp.width + x;
    const float4 cp = cin[i];
    if (!vr_surface(cp.w))
    {
        if (LAST)
        {
            out[i] = color[i];
            if (momentsOut)
                momentsOut[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        else
            cout[i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        return;
    }
    const float4 gp = g0[i];
    const float2 pp = g1[i];
    const int W = (int)vp.width, H = (int)vp.height, s = (int)vp.step;
    // vbar: the 3 x 3 Gaussian of the variance around p, offsets not dilated
    const float gk[3] = { 0.25f, 0.5f, 0.25f }; // (products of these are the kernel's 1/16, 1/8, 1/4: exact)
    float bv = 0.0f, bk = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
    {
        const int qy = (int)y + dy;
        const bool rowIn = qy >= 0 && qy < H;
        const uint32_t row = (uint32_t)(rowIn ? qy : (int)y) * vp.width;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
        {
            const int qx = (int)x + dx;
            const bool in = rowIn && qx >= 0 && qx < W;
            const float vq = cin[row + (uint32_t)(in ? qx : (int)x)].w;
            const float k = gk[dx + 1] * gk[dy + 1];
            if (in && vr_surface(vq))
            {
                bv = bv + k * vq;
                bk = bk + k;
            }
        }
    }
    const float vbar = bv / bk; // (the centre is always taken: bk > 0)
    const float kl = 1.0f / (vp.sigmaLuminance * sqrtf(vbar) + vp.epsilon);
    const float lp = vr_lum(cp.x, cp.y, cp.z);
    const float hk[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy)
    {
        const int qy = (int)y + dy * s;
        const bool rowIn = qy >= 0 && qy < H;
        const uint32_t row = (uint32_t)(rowIn ? qy : (int)y) * vp.width;
        const float hy = hk[dy + 2];
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
        {
            const int qx = (int)x + dx * s;
            const bool in = rowIn && qx >= 0 && qx < W;
            const uint32_t j = row + (uint32_t)(in ? qx : (int)x); // (a tap outside reads the row's centre column: a legal address, a value never used)
            const float4 cq = cin[j];
            float tn, tp;
            vr_guides(gp, pp, g0[j], g1[j], vp.kn, vp.kp, tn, tp);
            const float tl = vp.lumOff ? 0.0f : fabsf(vr_lum(cq.x, cq.y, cq.z) - lp) * kl;
            float a = (tl + tn) + tp;
            a = a <= 64.0f ? a : 64.0f; // (a NaN too)
            const float w = (hk[dx + 2] * hy) * skm::expf_(-a);
            if (in && vr_surface(cq.w)) // selected, never multiplied by zero
            {
                sw = sw + w;
                sx = sx + w * cq.x;
                sy = sy + w * cq.y;
                sz = sz + w * cq.z;
                sv = sv + (w * w) * cq.w;
            }
        }
    }
    float rx = sx / sw, ry = sy / sw, rz = sz / sw; // (the centre tap is always taken: sw > 0)
    const float rv = sv / (sw * sw);
    if (LAST)
    {
        if (vp.flags & SKH_DENOISE_REMODULATE)
        {
            const float4 al = albedo[i];
            rx = rx * dn_floor(al.x, vp.albedoFloor), ry = ry * dn_floor(al.y, vp.albedoFloor), rz = rz * dn_floor(al.z, vp.albedoFloor);
        }
        // (the moments record is read before the image is written: d_moments_out may be d_moments, a pixel reads only its own record)
        if (momentsOut)
        {
            const float4 m = moments[i];
            momentsOut[i] = make_float4(m.x, m.y, rv, m.w);
        }
        out[i] = make_uint4(__float_as_uint(rx), __float_as_uint(ry), __float_as_uint(rz), color[i].w);
    }
    else
        cout[i] = make_float4(rx, ry, rz, rv);
}

} // namespace skh
