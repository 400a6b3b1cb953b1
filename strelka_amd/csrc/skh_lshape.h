// strelka_hip -- light shapes: the sampled disk light and the UsdLux shaping cone (skh_set_light_shapes; DESIGN.md section 2 "Light shapes").
//
// Written once, for the device (k_shade's LSHAPE builds, skh_light_shape_probe) and for host programs (plain C++, no HIP header needed:
// tests/cpp/skhlshape_main.cpp).  Plain floats in, plain floats out; every operation is an IEEE single-precision + - * / sqrt (both sides compile
// without contraction) or skh_libm.h's pow, so both sides return the same bits.
//
//   the cone   c = dot(axis, w), w the unit direction from the light point to the shaded point.  s(c) = 0 unless c > cos_outer; otherwise
//              t = min((c - cos_outer) / (cos_inner - cos_outer), 1) (1 for a hard edge, cos_inner == cos_outer),
//              s = t^2 (3 - 2 t) * (focus > 0 ? pow(max(c, 0), focus) : 1)
//   the disk   the 16-gon rays can hit, not the analytic disc: v_k = O + cos(2 pi k / 16) X + sin(2 pi k / 16) Y, area 8 sin(pi / 8) |X x Y|.
//              A draw (ux, uy) selects sector k = min(int(16 ux), 15), u' = 16 ux - k (exact in fp32), and a uniform point of the triangle
//              (O, v_k, v_k+1) by the mapping the emitter table uses: su = sqrt(u'), (1 - su) O + su (1 - uy) v_k + su uy v_k+1
//   the pdf    per solid angle, the rect light's: dist^2 / (cos at the light * area); 0 from behind
#pragma once
#include <math.h>
#include <stdint.h>
#include "skh_libm.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SKH_LSHAPE_HD __host__ __device__ static inline
#else
#define SKH_LSHAPE_HD static inline
#endif

namespace skh
{

#define SKH_LSHAPE_SAMPLE_DISC 1u // == SKH_LIGHT_SHAPE_SAMPLE_DISC
#define SKH_LSHAPE_CONE 2u // == SKH_LIGHT_SHAPE_CONE
#define SKH_LSHAPE_SECTORS 16u
#define SKH_LSHAPE_AREA_FACTOR 3.0614674589207183f // 8 sin(pi / 8): the unit 16-gon's area

SKH_LSHAPE_HD float lshape_s(float c, float cosOuter, float cosInner, float focus)
{
    if (!(c > cosOuter)) // (a NaN is dark)
        return 0.0f;
    float t = 1.0f;
    if (cosInner > cosOuter)
    {
        t = (c - cosOuter) / (cosInner - cosOuter);
        t = t < 1.0f ? t : 1.0f;
    }
    const float smooth = (t * t) * (3.0f - 2.0f * t);
    return focus > 0.0f ? smooth * skm::powf_(c > 0.0f ? c : 0.0f, focus) : smooth;
}

// k = min(int(16 ux), 15), u' = 16 ux - k: the product by 16 and the difference of two floats of one binade or less apart are exact
SKH_LSHAPE_HD void lshape_sector(float ux, uint32_t& k, float& uPrime)
{
    const float s = (float)SKH_LSHAPE_SECTORS * ux;
    const int ki = (int)s;
    k = ki < 0 ? 0u : ((uint32_t)ki < SKH_LSHAPE_SECTORS - 1u ? (uint32_t)ki : SKH_LSHAPE_SECTORS - 1u);
    uPrime = s - (float)k;
}

// cos / sin of 2 pi k / 16, k = 0 .. 16, correctly rounded, with the symmetries of the circle kept exactly
SKH_LSHAPE_HD void lshape_cs(uint32_t k, float& c, float& s)
{
    const float a = 0.92387953251128674f, b = 0.70710678118654752f, d = 0.38268343236508977f;
    k &= 15u;
    const uint32_t quad = k >> 2, r = k & 3u;
    const float cq = r == 0u ? 1.0f : (r == 1u ? a : (r == 2u ? b : d)), sq = r == 0u ? 0.0f : (r == 1u ? d : (r == 2u ? b : a)); // the first quadrant
    switch (quad)
    {
    case 0:
        c = cq, s = sq;
        break;
    case 1:
        c = -sq, s = cq;
        break;
    case 2:
        c = -cq, s = -sq;
        break;
    default:
        c = sq, s = -cq;
        break;
    }
}

SKH_LSHAPE_HD void lshape_vertex(const float O[3], const float X[3], const float Y[3], uint32_t k, float v[3])
{
    float c, s;
    lshape_cs(k, c, s);
    for (int i = 0; i < 3; ++i)
        v[i] = (O[i] + c * X[i]) + s * Y[i];
}

// the sampled point of the 16-gon for the draw (ux, uy); returns the sector
SKH_LSHAPE_HD uint32_t lshape_disc_point(const float O[3], const float X[3], const float Y[3], float ux, float uy, float p[3])
{
    uint32_t k;
    float up;
    lshape_sector(ux, k, up);
    float v1[3], v2[3];
    lshape_vertex(O, X, Y, k, v1);
    lshape_vertex(O, X, Y, k + 1u, v2);
    const float su = sqrtf(up);
    const float b0 = 1.0f - su, b1 = su * (1.0f - uy), b2 = su * uy;
    for (int i = 0; i < 3; ++i)
        p[i] = (O[i] * b0 + v1[i] * b1) + v2[i] * b2;
    return k;
}

SKH_LSHAPE_HD float lshape_disc_area(const float X[3], const float Y[3])
{
    const float cx = X[1] * Y[2] - X[2] * Y[1], cy = X[2] * Y[0] - X[0] * Y[2], cz = X[0] * Y[1] - X[1] * Y[0];
    return SKH_LSHAPE_AREA_FACTOR * sqrtf((cx * cx + cy * cy) + cz * cz);
}

// per solid angle: dist^2 / (cosL * area), cosL the cosine at the light between its normal and the direction to the shaded point; 0 from behind
SKH_LSHAPE_HD float lshape_area_pdf(float dist, float cosL, float area)
{
    return cosL > 0.0f ? (dist * dist) / (cosL * area) : 0.0f; // (a NaN cosine fails the test)
}

} // namespace skh
