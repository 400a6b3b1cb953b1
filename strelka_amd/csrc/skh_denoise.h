// skh_denoise.h -- the edge-avoiding a-trous filter (skh_denoise; include/strelka_hip.h and DESIGN.md section 2 "Denoiser" are the definition).
//
//   k_dn_pack    one pass over the caller's five images -> per pixel a 16-byte colour record {rgb or demodulated rgb, surface flag} and a 24-byte guide record
//                {N.xyz, P.x}, {P.y, P.z}: a tap costs 40 bytes instead of 80 and never looks at IDS again.  Every word is a copy of a float32 of the definition
//                (the flag is 1.0f / 0.0f): the packing is lossless.
//   k_dn_level   one level, launched once per level, ping-ponging two colour images; the last launch writes the caller's image: remodulation, the alpha word and
//                the pixels that are not surface pixels (copied from the caller's input bit for bit) are folded into it.  No pass of their own.
//
// A workgroup is 64 x 4 pixels: a wave is 64 consecutive pixels of one row, so that each of its loads is one 1024-byte (colour, N) or 512-byte (P.yz) row segment.
// No LDS, no atomics.  The 25 taps are summed in the definition's order (dy outer, dx inner); a tap outside the image or on a pixel that is no surface pixel is
// SELECTED out (its address is clamped into the image so that the load is legal, its value never enters a sum).
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_kernels.h"

namespace skh
{

struct DnP // by-value kernel argument
{
    uint32_t width, height;
    uint32_t step;     // 1 << level
    float kc, kn, kp;  // 1 / (sigma_color * 2^-level)^2, 1 / sigma_normal^2, 1 / sigma_plane^2: rounded on the host (a product and a quotient each)
    float albedoFloor;
    uint32_t flags;    // k_dn_pack: SKH_DENOISE_DEMODULATE; k_dn_level<true>: SKH_DENOISE_REMODULATE
};

SKH_DI bool dn_finite(float x)
{
    return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}
// the definition's max(albedo, floor): a NaN albedo gives the floor
SKH_DI float dn_floor(float a, float f)
{
    return a > f ? a : f;
}

__global__ void __launch_bounds__(256) k_dn_pack(DnP dp, const float4* __restrict__ color, const uint4* __restrict__ ids, const float4* __restrict__ normal,
                                                  const float4* __restrict__ position, const float4* __restrict__ albedo, float4* __restrict__ c0,
                                                  float4* __restrict__ g0, float2* __restrict__ g1)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dp.width * dp.height)
        return;
    const float4 c = color[i];
    const uint32_t kind = ids[i].w;
    const bool surface = (kind == 1u || kind == 2u) && dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z);
    float4 rc = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rg = rc;
    float2 rp = make_float2(0.0f, 0.0f);
    if (surface)
    {
        rc = make_float4(c.x, c.y, c.z, 1.0f);
        if (dp.flags & SKH_DENOISE_DEMODULATE)
        {
            const float4 a = albedo[i];
            rc.x = c.x / dn_floor(a.x, dp.albedoFloor), rc.y = c.y / dn_floor(a.y, dp.albedoFloor), rc.z = c.z / dn_floor(a.z, dp.albedoFloor);
        }
        const float4 n = normal[i], p = position[i];
        rg = make_float4(n.x, n.y, n.z, p.x);
        rp = make_float2(p.y, p.z);
    }
    c0[i] = rc;
    g0[i] = rg;
    g1[i] = rp;
}

// LAST: this launch writes the caller's image (uint4 words: the pixels it passes through are bit copies)
template <bool LAST>
__global__ void __launch_bounds__(256) k_dn_level(DnP dp, const float4* __restrict__ cin, const float4* __restrict__ g0, const float2* __restrict__ g1,
                                                   float4* __restrict__ cout, const uint4* color, const float4* __restrict__ albedo, uint4* out)
{
    // (a one-dimensional grid of row-major 64 x 4 tiles: a 1 x 2^26 image has more tile rows than a grid has y blocks)
    const uint32_t tilesX = (dp.width + 63u) / 64u, ty = blockIdx.x / tilesX;
    const uint32_t x = (blockIdx.x - ty * tilesX) * 64u + threadIdx.x, y = ty * 4u + threadIdx.y;
    if (x >= dp.width || y >= dp.height)
        return;
    const uint32_t i = y * dp.width + x;
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
        const int qy = (int)y + dy * s;
        const bool rowIn = qy >= 0 && qy < H;
        const uint32_t row = (uint32_t)(rowIn ? qy : (int)y) * dp.width;
        const float hy = hk[dy + 2];
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
        {
            const int qx = (int)x + dx * s;
            const bool in = rowIn && qx >= 0 && qx < W;
            const uint32_t j = row + (uint32_t)(in ? qx : (int)x); // (a tap outside reads the row's centre column: a legal address, a value never used)
            const float4 cq = cin[j];
            const float4 gq = g0[j];
            const float2 pq = g1[j];
            const float ex = cq.x - cp.x, ey = cq.y - cp.y, ez = cq.z - cp.z;
            const float tc = ((ex * ex + ey * ey) + ez * ez) * dp.kc;
            const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
            const float tn = ((nx * nx + ny * ny) + nz * nz) * dp.kn;
            const float px = gq.w - gp.w, py = pq.x - pp.x, pz = pq.y - pp.y;
            const float d = (gp.x * px + gp.y * py) + gp.z * pz;
            const float tp = (d * d) * dp.kp;
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
            const float4 al = albedo[i];
            rx = rx * dn_floor(al.x, dp.albedoFloor), ry = ry * dn_floor(al.y, dp.albedoFloor), rz = rz * dn_floor(al.z, dp.albedoFloor);
        }
        out[i] = make_uint4(__float_as_uint(rx), __float_as_uint(ry), __float_as_uint(rz), color[i].w);
    }
    else
        cout[i] = make_float4(rx, ry, rz, 1.0f);
}

} // namespace skh
