// skh_temporal.h -- temporal accumulation (skh_temporal; include/strelka_hip.h and DESIGN.md section 2 "Temporal accumulation" are the definition).
//
//   k_tp_reproject   one lane, one pixel: projects the pixel's first-hit position into the previous frame, gathers the four bilinear taps of the previous
//                    history and guide planes, decides per tap, blends, and writes the output image, the new history and (optionally) the motion plane.
//
// A workgroup is 64 x 4 pixels as in k_dn_level: a wave is 64 consecutive pixels of one row, so that each load of a current plane is one 1024-byte row segment.
// No LDS, no atomics, no scratch.  The sixteen previous-frame loads (4 taps x history, ids, normal, position) go out with clamped addresses before the first of
// them is used; a tap that is not accepted is SELECTED out afterwards (its value never enters a sum).  The only branches are uniform ones (flags, a previous
// frame or none, a motion plane or none) and the exit of pixels that are no surface pixels.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_denoise.h"

namespace skh
{

struct TpP // by-value kernel argument
{
    uint32_t width, height;
    float prevWorldToClip[16];
    float normalMin, planeTolerance, maxHistory, initialLength, albedoFloor;
    uint32_t flags;   // SKH_TEMPORAL_DEMODULATE
    uint32_t hasPrev; // 0: no previous frame (the four previous-frame pointers are not read)
};

// `color` and `out` may be the same image: a pixel reads its own record only, and before it writes
__global__ void __launch_bounds__(256) k_tp_reproject(TpP tp, const uint4* color, const uint4* __restrict__ ids, const float4* __restrict__ normal,
                                                       const float4* __restrict__ position, const float4* __restrict__ albedo,
                                                       const float4* __restrict__ prevHistory, const uint4* __restrict__ prevIds,
                                                       const float4* __restrict__ prevNormal, const float4* __restrict__ prevPosition, uint4* out,
                                                       float4* __restrict__ historyOut, float4* __restrict__ motion)
{
    // (a one-dimensional grid of row-major 64 x 4 tiles, as k_dn_level's)
    const uint32_t tilesX = (tp.width + 63u) / 64u, tileY = blockIdx.x / tilesX;
    const uint32_t x = (blockIdx.x - tileY * tilesX) * 64u + threadIdx.x, y = tileY * 4u + threadIdx.y;
    if (x >= tp.width || y >= tp.height)
        return;
    const uint32_t i = y * tp.width + x;
    const uint4 cw = color[i];
    const uint4 id = ids[i];
    const float cr = __uint_as_float(cw.x), cg = __uint_as_float(cw.y), cb = __uint_as_float(cw.z);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!((id.w == 1u || id.w == 2u) && dn_finite(cr) && dn_finite(cg) && dn_finite(cb))) // not a surface pixel
    {
        out[i] = cw;
        historyOut[i] = zero;
        if (motion)
            motion[i] = zero;
        return;
    }
    const float4 N = normal[i], P = position[i];
    const bool demodulate = (tp.flags & SKH_TEMPORAL_DEMODULATE) != 0u;
    float mx = 1.0f, my = 1.0f, mz = 1.0f, cx = cr, cy = cg, cz = cb;
    if (demodulate)
    {
        const float4 a = albedo[i];
        mx = dn_floor(a.x, tp.albedoFloor), my = dn_floor(a.y, tp.albedoFloor), mz = dn_floor(a.z, tp.albedoFloor);
        cx = cr / mx, cy = cg / my, cz = cb / mz;
    }
    float ix_ = cx, iy_ = cy, iz_ = cz, nn = tp.initialLength; // the pixel without history
    float4 mv = zero;
    if (tp.hasPrev)
    {
        const float W = (float)tp.width, H = (float)tp.height; // (exact: <= 2^26)
        const v4 clip = mul44(tp.prevWorldToClip, mk4(P.x, P.y, P.z, 1.0f));
        const float fx = ((clip.x / clip.w) * 0.5f + 0.5f) * W - 0.5f;
        const float fy = ((clip.y / clip.w) * 0.5f + 0.5f) * H - 0.5f;
        // (every comparison false for a NaN; the range test before the conversion to an integer)
        const bool projects = clip.w > 0.0f && dn_finite(fx) && dn_finite(fy) && fx >= -1.0f && fx <= W && fy >= -1.0f && fy <= H;
        const float gx = projects ? fx : (float)x, gy = projects ? fy : (float)y; // (a pixel that does not project gathers around itself: legal, never used)
        const float flx = floorf(gx), fly = floorf(gy);
        const int qx0 = (int)flx, qy0 = (int)fly; // -1 .. W, -1 .. H
        const float tx = gx - flx, ty = gy - fly;
        const float ux = 1.0f - tx, uy = 1.0f - ty;
        const float w[4] = { ux * uy, tx * uy, ux * ty, tx * ty };
        const int Wi = (int)tp.width, Hi = (int)tp.height;
        float4 hq[4], nq[4], pq[4];
        uint4 iq[4];
        bool in[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const int qx = qx0 + (k & 1), qy = qy0 + (k >> 1);
            in[k] = qx >= 0 && qx < Wi && qy >= 0 && qy < Hi;
            const int ax = qx < 0 ? 0 : (qx < Wi ? qx : Wi - 1), ay = qy < 0 ? 0 : (qy < Hi ? qy : Hi - 1);
            const uint32_t j = (uint32_t)ay * tp.width + (uint32_t)ax;
            hq[k] = prevHistory[j];
            iq[k] = prevIds[j];
            nq[k] = prevNormal[j];
            pq[k] = prevPosition[j];
        }
        float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sn = 0.0f;
        uint32_t mask = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const float dn = (nq[k].x * N.x + nq[k].y * N.y) + nq[k].z * N.z;
            const float ex = pq[k].x - P.x, ey = pq[k].y - P.y, ez = pq[k].z - P.z;
            const float d = (N.x * ex + N.y * ey) + N.z * ez;
            const bool accepted = projects && in[k] && w[k] > 0.0f && iq[k].w == id.w && iq[k].x == id.x && dn_finite(hq[k].x) && dn_finite(hq[k].y) &&
                                  dn_finite(hq[k].z) && dn_finite(hq[k].w) && hq[k].w >= 1.0f && dn >= tp.normalMin && fabsf(d) <= tp.planeTolerance;
            // selected, never multiplied by zero
            sw = accepted ? sw + w[k] : sw;
            sx = accepted ? sx + w[k] * hq[k].x : sx;
            sy = accepted ? sy + w[k] * hq[k].y : sy;
            sz = accepted ? sz + w[k] * hq[k].z : sz;
            sn = accepted ? sn + w[k] * hq[k].w : sn;
            mask |= accepted ? (1u << k) : 0u;
        }
        // (computed by every lane, 0 / 0 included, and selected: no branch on what the taps were)
        const float hx = sx / sw, hy = sy / sw, hz = sz / sw, nh = sn / sw;
        const float n1 = nh + 1.0f;
        const float nb = n1 < tp.maxHistory ? n1 : tp.maxHistory;
        const float alpha = 1.0f / nb;
        const bool any = mask != 0u;
        ix_ = any ? hx + (cx - hx) * alpha : cx, iy_ = any ? hy + (cy - hy) * alpha : cy, iz_ = any ? hz + (cz - hz) * alpha : cz;
        nn = any ? nb : tp.initialLength;
        if (projects)
            mv = make_float4(fx - (float)x, fy - (float)y, sw, (float)mask);
    }
    historyOut[i] = make_float4(ix_, iy_, iz_, nn);
    if (demodulate)
        ix_ = ix_ * mx, iy_ = iy_ * my, iz_ = iz_ * mz;
    out[i] = make_uint4(__float_as_uint(ix_), __float_as_uint(iy_), __float_as_uint(iz_), cw.w);
    if (motion)
        motion[i] = mv;
}

} // namespace skh
