// skh_motion.h -- object motion for the temporal passes (skh_rewind_guides; include/strelka_hip.h and DESIGN.md section 2 "Object motion" are the definition).
//
//   k_mo_rewind   one lane, one pixel: expresses the pixel's first-hit position and normal in the previous frame's world, through the motion entry of the
//                 pixel's instance.  skh_temporal and skh_moments, handed the two planes it writes, then follow a moved instance with no change of their own.
//
// Workgroups and the grid are skh_image.h's.
// No LDS, no atomics, no scratch.  The six float4 of the table entry are gathered with the index clamped to a legal entry, before the first of them is used; where
// the entry does not apply the pixel's own words are SELECTED (as words: a NaN keeps its payload).  The only branch is the exit at the image's edge.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_image.h"

namespace skh
{

// `position` / `positionOut` and `normal` / `normalOut` may be the same planes: a pixel reads its own records only, and before it writes.  n >= 1.
__global__ void __launch_bounds__(256) k_mo_rewind(uint32_t width, uint32_t height, uint32_t n, const float4* __restrict__ table, const uint4* __restrict__ ids,
                                                    const float4* position, const float4* normal, float4* positionOut, float4* normalOut)
{
    uint32_t x, y, i;
    if (!img_pixel(width, height, x, y, i))
        return;
    const uint4 id = ids[i];
    const float4 P = position[i], N = normal[i];
    const uint32_t e = id.x < n ? id.x : n - 1u; // (a legal entry whatever the pixel holds)
    const float4* t = table + (size_t)e * 6u;
    const float4 m0 = t[0], m1 = t[1], m2 = t[2], k0 = t[3], k1 = t[4], k2 = t[5]; // k0 = {k0 k1 k2 k3}, k1 = {k4 .. k7}, k2 = {k8, flags, 0, 0}
    const uint32_t flags = __float_as_uint(k2.y);
    const bool applies = (id.w == 1u || id.w == 2u) && id.x < n && (flags & SKH_MOTION_MOVED) != 0u;
    const bool drop = (flags & SKH_MOTION_DROP) != 0u;
    const float px = ((m0.x * P.x + m0.y * P.y) + m0.z * P.z) + m0.w;
    const float py = ((m1.x * P.x + m1.y * P.y) + m1.z * P.z) + m1.w;
    const float pz = ((m2.x * P.x + m2.y * P.y) + m2.z * P.z) + m2.w;
    const float vx = (k0.x * N.x + k0.y * N.y) + k0.z * N.z;
    const float vy = (k0.w * N.x + k1.x * N.y) + k1.y * N.z;
    const float vz = (k1.z * N.x + k1.w * N.y) + k2.x * N.z;
    const float s = (vx * vx + vy * vy) + vz * vz;
    const float r = sqrtf(s);
    const uint32_t qnan = 0x7fc00000u;
    const bool moved = applies && !drop;
    uint4 po, no;
    po.x = applies ? (drop ? qnan : __float_as_uint(px)) : __float_as_uint(P.x);
    po.y = applies ? (drop ? qnan : __float_as_uint(py)) : __float_as_uint(P.y);
    po.z = applies ? (drop ? qnan : __float_as_uint(pz)) : __float_as_uint(P.z);
    po.w = __float_as_uint(P.w);
    no.x = moved ? __float_as_uint(vx / r) : __float_as_uint(N.x);
    no.y = moved ? __float_as_uint(vy / r) : __float_as_uint(N.y);
    no.z = moved ? __float_as_uint(vz / r) : __float_as_uint(N.z);
    no.w = __float_as_uint(N.w);
    reinterpret_cast<uint4*>(positionOut)[i] = po;
    reinterpret_cast<uint4*>(normalOut)[i] = no;
}

} // namespace skh
