// strelka_hip -- the random draw of fractional opacity (skh_set_material_blend; DESIGN.md section 2 "Fractional opacity").
//
// Written once, for the device (k_cutout's BLEND build, skh_blend_probe) and for host programs (plain C++, no HIP header needed).
// A radiance ray takes a blend hit of opacity a iff blend_xi(sampleIdx, depth, round) < a:
//   sampleIdx  the sampler's: encode_morton2(px, py) * sppTotal + pixel sample index (init_sampler)
//   depth      the bounce whose trace launch produced the hit record
//   round      the number of hits this ray has already passed (0 in the stage's first launch, r + 1 after continuation round r)
// A pure function of the path's identity and the ray's progress: no state, no atomics, nothing that depends on which lane, launch or sub-frame batch
// evaluates it.  White noise -- the sampler's five Sobol dimensions are all taken.  The mixing steps are the sampler's own hash_murmur / hash_combine
// (RandomSampler.h:86-95, 50-53), restated here so that this header stands alone; the salt keeps the draw apart from the sampler's scramble seeds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SKH_BLEND_HD __host__ __device__ static inline
#else
#define SKH_BLEND_HD static inline
#endif

namespace skh
{

#define SKH_BLEND_SALT 0xb5297a4du

SKH_BLEND_HD uint32_t blend_murmur(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
SKH_BLEND_HD uint32_t blend_combine(uint32_t seed, uint32_t v)
{
    return seed ^ (v + (seed << 6) + (seed >> 2));
}
SKH_BLEND_HD uint32_t blend_hash(uint32_t sampleIdx, uint32_t depth, uint32_t round)
{
    return blend_murmur(blend_combine(blend_combine(blend_murmur(sampleIdx ^ SKH_BLEND_SALT), depth), round));
}
// 24 bits: every value is a float, xi < 1, and xi < a is the comparison of two floats without a rounding in between
SKH_BLEND_HD float blend_xi(uint32_t sampleIdx, uint32_t depth, uint32_t round)
{
    return (float)(blend_hash(sampleIdx, depth, round) >> 8) * 0x1p-24f;
}

} // namespace skh
