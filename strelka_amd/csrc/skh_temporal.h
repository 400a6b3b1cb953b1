// skh_temporal.h -- temporal accumulation (skh_temporal; include/strelka_hip.h and DESIGN.md section 2 "Temporal accumulation" are the definition).
//
//   k_tp_reproject   one lane, one pixel: projects the pixel's first-hit position into the previous frame, gathers the four bilinear taps of the previous
//                    history and guide planes, decides per tap, blends, and writes the output image, the new history and (optionally) the motion plane.
//
// Workgroups, the grid and the reprojection footprint are skh_image.h's.  No LDS, no atomics, no scratch.  The sixteen previous-frame loads (4 taps x history,
// ids, normal, position) go out with the footprint's clamped addresses before the first of them is used; a tap that is not accepted is SELECTED out afterwards
// (its value never enters a sum).  The only branches are uniform ones (flags, a previous
// frame or none, a motion plane or none) and the exit of pixels that are no surface pixels.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_image.h"

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
    uint32_t x, y, i;
    if (!img_pixel(tp.width, tp.height, x, y, i))
        return;
    const uint4 cw = color[i];
    const uint4 id = ids[i];
    const float cr = __uint_as_float(cw.x), cg = __uint_as_float(cw.y), cb = __uint_as_float(cw.z);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!img_surface(id.w, cr, cg, cb)) // not a surface pixel
    {
        out[i] = cw;
        historyOut[i] = zero;
        if (motion)
            motion[i] = zero;
        return;
    }
    const float4 N = normal[i], P = position[i];
    const bool demodulate = (tp.flags & SKH_TEMPORAL_DEMODULATE) != 0u;
    float3 m = make_float3(1.0f, 1.0f, 1.0f);
    float cx = cr, cy = cg, cz = cb;
    if (demodulate)
    {
        m = img_albedo(albedo[i], tp.albedoFloor);
        cx = cr / m.x, cy = cg / m.y, cz = cb / m.z;
    }
    float ix_ = cx, iy_ = cy, iz_ = cz, nn = tp.initialLength; // the pixel without history
    float4 mv = zero;
    if (tp.hasPrev)
    {
        const ImgFootprint f = img_footprint(tp.prevWorldToClip, tp.width, tp.height, P, x, y);
        float4 hq[4], nq[4], pq[4];
        uint4 iq[4];
        bool in[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            uint32_t j;
            in[k] = img_footprint_tap(f, k, tp.width, tp.height, j);
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
            const bool accepted = f.projects && in[k] && f.w[k] > 0.0f && iq[k].w == id.w && iq[k].x == id.x && dn_finite(hq[k].x) && dn_finite(hq[k].y) &&
                                  dn_finite(hq[k].z) && dn_finite(hq[k].w) && hq[k].w >= 1.0f && dn >= tp.normalMin && fabsf(d) <= tp.planeTolerance;
            // selected, never multiplied by zero
            sw = accepted ? sw + f.w[k] : sw;
            sx = accepted ? sx + f.w[k] * hq[k].x : sx;
            sy = accepted ? sy + f.w[k] * hq[k].y : sy;
            sz = accepted ? sz + f.w[k] * hq[k].z : sz;
            sn = accepted ? sn + f.w[k] * hq[k].w : sn;
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
        if (f.projects)
            mv = make_float4(f.fx - (float)x, f.fy - (float)y, sw, (float)mask);
    }
    historyOut[i] = make_float4(ix_, iy_, iz_, nn);
    if (demodulate)
        ix_ = ix_ * m.x, iy_ = iy_ * m.y, iz_ = iz_ * m.z;
    out[i] = make_uint4(__float_as_uint(ix_), __float_as_uint(iy_), __float_as_uint(iz_), cw.w);
    if (motion)
        motion[i] = mv;
}

} // namespace skh
