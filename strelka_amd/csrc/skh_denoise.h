// skh_denoise.h -- the edge-avoiding a-trous filter (skh_denoise; include/strelka_hip.h and DESIGN.md section 2 "Denoiser" are the definition).
//
//   k_img_pack<false>  (skh_image.h) packs the caller's five images: the surface flag 1.0f / 0.0f in the colour record's fourth word.
//   k_dn_level         one level, launched once per level, ping-ponging two colour images; the last launch writes the caller's image: remodulation, the alpha word and
//                      the pixels that are not surface pixels (copied from the caller's input bit for bit) are folded into it.  No pass of their own.
//
// Workgroups, the grid and the clamped taps are skh_image.h's.  No LDS, no atomics.  The 25 taps are summed in the definition's order (dy outer, dx inner); a tap
// outside the image or on a pixel that is no surface pixel is SELECTED out.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_image.h"

namespace skh
{

struct DnP // by-value kernel argument
{
    uint32_t width, height;
    uint32_t step;     // 1 << level
    float kc, kn, kp;  // 1 / (sigma_color * 2^-level)^2, 1 / sigma_normal^2, 1 / sigma_plane^2: rounded on the host (a product and a quotient each)
    float albedoFloor;
    uint32_t flags;    // k_dn_level<true>: SKH_DENOISE_REMODULATE
};

// LAST: this launch writes the caller's image (uint4 words: the pixels it passes through are bit copies)
template <bool LAST>
__global__ void __launch_bounds__(256) k_dn_level(DnP dp, const float4* __restrict__ cin, const float4* __restrict__ g0, const float2* __restrict__ g1,
                                                   float4* __restrict__ cout, const uint4* color, const float4* __restrict__ albedo, uint4* out)
{
    uint32_t x, y, i;
    if (!img_pixel(dp.width, dp.height, x, y, i))
        return;
    const float4 cp = cin[i];
    if (cp.w == 0.0f) // not a surface pixel
    {
        if (LAST)
            out[i] = color[i];
        else
            cout[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 gp = g0[i];
    const float2 pp = g1[i];
    const float hk[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    const int W = (int)dp.width, H = (int)dp.height, s = (int)dp.step;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy)
    {
        const ImgRow row = img_row(y, dy * s, dp.width, H);
        const float hy = hk[dy + 2];
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
        {
            uint32_t j;
            const bool in = img_tap(row, x, dx * s, W, j);
            const float4 cq = cin[j];
            const float ex = cq.x - cp.x, ey = cq.y - cp.y, ez = cq.z - cp.z;
            const float tc = ((ex * ex + ey * ey) + ez * ez) * dp.kc;
            float tn, tp;
            img_guides(gp, pp, g0[j], g1[j], dp.kn, dp.kp, tn, tp);
            float a = (tc + tn) + tp;
            a = a <= 64.0f ? a : 64.0f; // (a NaN too)
            const float w = (hk[dx + 2] * hy) * skm::expf_(-a);
            if (in && cq.w != 0.0f) // selected, never multiplied by zero
            {
                sw = sw + w;
                sx = sx + w * cq.x;
                sy = sy + w * cq.y;
                sz = sz + w * cq.z;
            }
        }
    }
    float rx = sx / sw, ry = sy / sw, rz = sz / sw; // (the centre tap is always taken: sw > 0)
    if (LAST)
    {
        if (dp.flags & SKH_DENOISE_REMODULATE)
        {
            const float3 al = img_albedo(albedo[i], dp.albedoFloor);
            rx = rx * al.x, ry = ry * al.y, rz = rz * al.z;
        }
        out[i] = make_uint4(__float_as_uint(rx), __float_as_uint(ry), __float_as_uint(rz), color[i].w);
    }
    else
        cout[i] = make_float4(rx, ry, rz, 1.0f);
}

} // namespace skh
