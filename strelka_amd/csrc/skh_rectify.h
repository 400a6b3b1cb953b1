// skh_rectify.h -- history rectification (skh_rectify; include/strelka_hip.h and DESIGN.md section 2 "History rectification" are the definition).
//
//   k_rc_rectify<R>   one lane, one pixel: gathers the (2R + 1)^2 window of the fast history around the pixel, takes the mean and the standard deviation of the
//                     taps on the pixel's own surface in two sweeps, clamps the pixel's long history to mean +- k sd per channel, and writes the output image,
//                     the long history to store and (optionally) the info plane.
//
// Workgroups, the grid and the clamped taps are skh_image.h's.  No LDS, no atomics, no scratch.  The plain gather of k_vr_estimate: the first sweep loads a tap's
// fast record and its ids record (16 bytes each: one full-width load per plane and tap) and keeps which taps it took as one bit each.  For the
// second sweep the 3 x 3 window's nine records stay in registers; the wider windows load the fast records again (they are in the cache the first sweep filled).
// Either way it SELECTS by those bits -- a skipped tap never enters a sum.  The only branches are uniform ones (an info plane or none) and the exit of pixels
// that are not rectified.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_image.h"

namespace skh
{

struct RcP // by-value kernel argument
{
    uint32_t width, height;
    float k, albedoFloor;
    uint32_t flags; // SKH_RECTIFY_*
    uint32_t kInf;  // k == +inf: nothing is clamped (selected, not inf * 0)
};

SKH_DI bool rc_record(const float4& f) // a history record with finite rgb and a finite length >= 1
{
    return dn_finite(f.x) && dn_finite(f.y) && dn_finite(f.z) && dn_finite(f.w) && f.w >= 1.0f;
}

// `image` / `out` and `history` / `historyOut` may be the same planes: a pixel reads its own records of those only, and before it writes.  `fast` is read
// around the pixel and is no output.
template <int R>
__global__ void __launch_bounds__(256) k_rc_rectify(RcP rp, const uint4* image, const uint4* __restrict__ ids, const float4* __restrict__ albedo,
                                                     const uint4* history, const float4* __restrict__ fast, uint4* out, uint4* historyOut,
                                                     float4* __restrict__ info)
{
    uint32_t x, y, i;
    if (!img_pixel(rp.width, rp.height, x, y, i))
        return;
    const uint4 cw = image[i], hw = history[i];
    const uint32_t inst = ids[i].x, kind = ids[i].w;
    const float4 h = make_float4(__uint_as_float(hw.x), __uint_as_float(hw.y), __uint_as_float(hw.z), __uint_as_float(hw.w));
    const float4 fp = fast[i];
    if (!((kind == 1u || kind == 2u) && rc_record(h) && rc_record(fp))) // not a rectified pixel: both records copied as words
    {
        out[i] = cw;
        historyOut[i] = hw;
        if (info)
            info[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const int W = (int)rp.width, H = (int)rp.height;
    constexpr int D = 2 * R + 1;
    constexpr int ROWS = R == 1 ? D : 1; // (the rows of the two wider windows stay a loop: unrolled, their 25 or 49 taps' flags spill scalar registers)
    constexpr bool KEEP = R == 1; // (the 3 x 3 window's nine records stay in registers for the second sweep; the wider windows gather again)
    float3 kept[KEEP ? D * D : 1];
    // first sweep: which taps are taken, their count and their sums
    uint64_t taken = 0u;
    float s0 = 0.0f, s1x = 0.0f, s1y = 0.0f, s1z = 0.0f;
#pragma unroll ROWS
    for (int dy = -R; dy <= R; ++dy)
    {
        const ImgRow row = img_row(y, dy, rp.width, H);
        uint32_t rowTaken = 0u;
#pragma unroll
        for (int dx = -R; dx <= R; ++dx)
        {
            uint32_t j;
            const bool in = img_tap(row, x, dx, W, j);
            const float4 f = fast[j];
            const uint4 iq = ids[j];
            const bool t = in && iq.w == kind && iq.x == inst && rc_record(f);
            if (KEEP)
                kept[(dy + R) * D + (dx + R)] = make_float3(f.x, f.y, f.z);
            // selected, never multiplied by zero
            s0 = t ? s0 + 1.0f : s0;
            s1x = t ? s1x + f.x : s1x, s1y = t ? s1y + f.y : s1y, s1z = t ? s1z + f.z : s1z;
            rowTaken |= t ? (1u << (dx + R)) : 0u;
        }
        taken |= (uint64_t)rowTaken << ((dy + R) * D);
    }
    const float mx = s1x / s0, my = s1y / s0, mz = s1z / s0; // (the centre is taken: s0 >= 1)
    // second sweep: the squared deviations from that mean, in the same order
    float s2x = 0.0f, s2y = 0.0f, s2z = 0.0f;
#pragma unroll ROWS
    for (int dy = -R; dy <= R; ++dy)
    {
        const ImgRow row = img_row(y, dy, rp.width, H);
        const uint32_t rowTaken = (uint32_t)(taken >> ((dy + R) * D));
#pragma unroll
        for (int dx = -R; dx <= R; ++dx)
        {
            uint32_t j;
            img_tap(row, x, dx, W, j);
            float3 f;
            if (KEEP)
                f = kept[(dy + R) * D + (dx + R)];
            else
            {
                const float4 g = fast[j];
                f = make_float3(g.x, g.y, g.z);
            }
            const bool t = ((rowTaken >> (dx + R)) & 1u) != 0u;
            const float ex = f.x - mx, ey = f.y - my, ez = f.z - mz;
            s2x = t ? s2x + ex * ex : s2x, s2y = t ? s2y + ey * ey : s2y, s2z = t ? s2z + ez * ez : s2z;
        }
    }
    const float sx = sqrtf(s2x / s0), sy = sqrtf(s2y / s0), sz = sqrtf(s2z / s0);
    // the clamp: every comparison false for a NaN; with k == +inf none is made
    const bool clamp = rp.kInf == 0u;
    const float ex = rp.k * sx, ey = rp.k * sy, ez = rp.k * sz;
    const float lox = mx - ex, loy = my - ey, loz = mz - ez, hix = mx + ex, hiy = my + ey, hiz = mz + ez;
    const bool bx = clamp && h.x < lox, by = clamp && h.y < loy, bz = clamp && h.z < loz;
    const bool ax = clamp && h.x > hix, ay = clamp && h.y > hiy, az = clamp && h.z > hiz;
    float rx = h.x, ry = h.y, rz = h.z;
    rx = bx ? lox : rx, ry = by ? loy : ry, rz = bz ? loz : rz;
    rx = ax ? hix : rx, ry = ay ? hiy : ry, rz = az ? hiz : rz;
    const uint32_t mask = ((bx || ax) ? 1u : 0u) | ((by || ay) ? 2u : 0u) | ((bz || az) ? 4u : 0u);
    const float nn = ((rp.flags & SKH_RECTIFY_SHORTEN) != 0u && mask != 0u && fp.w < h.w) ? fp.w : h.w;
    historyOut[i] = make_uint4(__float_as_uint(rx), __float_as_uint(ry), __float_as_uint(rz), __float_as_uint(nn));
    float ox = rx, oy = ry, oz = rz;
    if (rp.flags & SKH_RECTIFY_REMODULATE)
    {
        const float3 a = img_albedo(albedo[i], rp.albedoFloor);
        ox = rx * a.x, oy = ry * a.y, oz = rz * a.z;
    }
    out[i] = make_uint4(__float_as_uint(ox), __float_as_uint(oy), __float_as_uint(oz), cw.w);
    if (info)
    {
        float dm = fabsf(rx - h.x);
        const float dy_ = fabsf(ry - h.y), dz_ = fabsf(rz - h.z);
        dm = dy_ > dm ? dy_ : dm;
        dm = dz_ > dm ? dz_ : dm;
        info[i] = make_float4((float)mask, s0, dm, nn);
    }
}

} // namespace skh
