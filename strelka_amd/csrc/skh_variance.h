// skh_variance.h -- variance guidance (skh_moments, skh_denoise_variance; include/strelka_hip.h and DESIGN.md section 2 "Variance guidance" are the definition).
//
//   k_vr_moments    one lane, one pixel: the luminance of the raw colour, its first two moments blended with the previous frame's through the taps skh_temporal
//                   accepted (the mask word of its motion plane), the variance.  The footprint is the one k_tp_reproject gathers through (skh_image.h).
//   k_img_pack<true>  (skh_image.h) packs with the variance in the colour record's fourth word: {rgb or demodulated rgb, v0}, v0 >= 0 on a surface pixel
//                   and -1 on every other.
//   k_vr_estimate   launched only with SKH_VDENOISE_ESTIMATE, from the packed colour image into the second one: a surface pixel whose moments are younger than
//                   min_history replaces v0 by the 7 x 7 estimate; every other record is copied.  (A pass of its own, into an image of its own: it reads its
//                   neighbours' records, so it must not write where it reads.)  The branch is taken by whole waves where a region was disoccluded.
//   k_vr_level      k_dn_level with the luminance stop 1 / (sigma sqrt(vbar) + epsilon) in place of the colour stop, and the variance filtered with the squared
//                   weights.  The last launch writes the caller's image and, when given, the moments record with the filtered variance.
//
// Workgroups, the grid, the clamped taps and the guide terms are skh_image.h's; skipped taps are selected out as in k_dn_level.  No LDS, no atomics, no scratch.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_image.h"
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
    uint32_t flags;         // k_vr_level<true>: SKH_DENOISE_REMODULATE
    uint32_t lumOff;        // sigma_luminance == +inf: the luminance term is 0, not inf * 0
};

SKH_DI float vr_lum(float r, float g, float b)
{
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
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
    uint32_t x, y, i;
    if (!img_pixel(tp.width, tp.height, x, y, i))
        return;
    const float4 c = color[i];
    if (!img_surface(ids[i].w, c.x, c.y, c.z)) // not a surface pixel
    {
        momentsOut[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float cx = c.x, cy = c.y, cz = c.z;
    if (tp.flags & SKH_TEMPORAL_DEMODULATE)
    {
        const float3 a = img_albedo(albedo[i], tp.albedoFloor);
        cx = c.x / a.x, cy = c.y / a.y, cz = c.z / a.z;
    }
    const float l = vr_lum(cx, cy, cz), ll = l * l;
    float m1 = l, m2 = ll, nn = tp.initialLength; // the pixel without history
    if (tp.hasPrev)
    {
        const float4 P = position[i];
        const float mw = motion[i].w;
        const uint32_t mask = (mw >= 0.0f && mw <= 15.0f) ? (uint32_t)mw : 0u; // (a NaN gives 0)
        const ImgFootprint f = img_footprint(tp.prevWorldToClip, tp.width, tp.height, P, x, y);
        float4 mq[4];
        bool in[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            uint32_t j;
            in[k] = img_footprint_tap(f, k, tp.width, tp.height, j);
            mq[k] = prevMoments[j];
        }
        float sw = 0.0f, s1 = 0.0f, s2 = 0.0f, sn = 0.0f;
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const bool used = f.projects && ((mask >> k) & 1u) != 0u && in[k] && f.w[k] > 0.0f && dn_finite(mq[k].x) && dn_finite(mq[k].y) && dn_finite(mq[k].w) &&
                              mq[k].w >= 1.0f;
            // selected, never multiplied by zero
            sw = used ? sw + f.w[k] : sw;
            s1 = used ? s1 + f.w[k] * mq[k].x : s1;
            s2 = used ? s2 + f.w[k] * mq[k].y : s2;
            sn = used ? sn + f.w[k] * mq[k].w : sn;
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
__global__ void __launch_bounds__(256) k_vr_estimate(VrP vp, const float4* __restrict__ cin, const float4* __restrict__ g0, const float2* __restrict__ g1,
                                                      const float4* __restrict__ moments, float4* __restrict__ cout)
{
    uint32_t x, y, i;
    if (!img_pixel(vp.width, vp.height, x, y, i))
        return;
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
                const ImgRow row = img_row(y, dy, vp.width, H);
#pragma unroll
                for (int dx = -3; dx <= 3; ++dx)
                {
                    uint32_t j;
                    const bool in = img_tap(row, x, dx, W, j);
                    const float cw = cin[j].w;
                    const float4 mq = moments[j];
                    float tn, tp;
                    img_guides(gp, pp, g0[j], g1[j], vp.kn, vp.kp, tn, tp);
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
    uint32_t x, y, i;
    if (!img_pixel(vp.width, vp.height, x, y, i))
        return;
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
        const ImgRow row = img_row(y, dy, vp.width, H);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
        {
            uint32_t j;
            const bool in = img_tap(row, x, dx, W, j);
            const float vq = cin[j].w;
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
        const ImgRow row = img_row(y, dy * s, vp.width, H);
        const float hy = hk[dy + 2];
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
        {
            uint32_t j;
            const bool in = img_tap(row, x, dx * s, W, j);
            const float4 cq = cin[j];
            float tn, tp;
            img_guides(gp, pp, g0[j], g1[j], vp.kn, vp.kp, tn, tp);
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
            const float3 al = img_albedo(albedo[i], vp.albedoFloor);
            rx = rx * al.x, ry = ry * al.y, rz = rz * al.z;
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
