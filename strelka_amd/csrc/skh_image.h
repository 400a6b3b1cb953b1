// skh_image.h -- the words the image passes are written in, and the one kernel two of them share: k_img_pack (skh_denoise.h, skh_temporal.h, skh_variance.h, skh_motion.h, skh_rectify.h; DESIGN.md section 2
// "Image passes").  Every function is forced inline and keeps the operation order of the definitions: a kernel written with them computes the bits it would
// compute with their bodies written out (no contraction, no fast-math).
//
// A workgroup is 64 x 4 pixels: a wave is 64 consecutive pixels of one row, so that each load of a plane is one 1024-byte row segment.  A tap that a pass does not
// take -- outside the image, or refused by the pass's own test -- is SELECTED out: its address is clamped into the image so that the load is legal, its value
// never enters a sum.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_kernels.h"

namespace skh
{

SKH_DI bool dn_finite(float x)
{
    return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}
// the definition's max(albedo, floor): a NaN albedo gives the floor
SKH_DI float dn_floor(float a, float f)
{
    return a > f ? a : f;
}

// the launch of a pass over a width x height image, block(64, 4): a one-dimensional grid of row-major 64 x 4 tiles (<= 2^24 + 2^20 of them: a 1 x 2^26 image
// has more tile rows than a grid has y blocks)
static inline dim3 img_grid(uint32_t width, uint32_t height)
{
    return dim3(((width + 63u) / 64u) * ((height + 3u) / 4u));
}
// this lane's pixel (x, y) and its index i in that grid; false beyond the image's edge
SKH_DI bool img_pixel(uint32_t width, uint32_t height, uint32_t& x, uint32_t& y, uint32_t& i)
{
    const uint32_t tilesX = (width + 63u) / 64u, tileY = blockIdx.x / tilesX;
    x = (blockIdx.x - tileY * tilesX) * 64u + threadIdx.x, y = tileY * 4u + threadIdx.y;
    i = y * width + x;
    return x < width && y < height;
}

// a surface pixel: the first hit is a triangle or a curve (kind 1 or 2) and the three colour words are finite
SKH_DI bool img_surface(uint32_t kind, float r, float g, float b)
{
    return (kind == 1u || kind == 2u) && dn_finite(r) && dn_finite(g) && dn_finite(b);
}

// the floored albedo of a pixel: the divisor of a demodulation, the factor of a remodulation
SKH_DI float3 img_albedo(const float4& a, float floor)
{
    return make_float3(dn_floor(a.x, floor), dn_floor(a.y, floor), dn_floor(a.z, floor));
}

// A window's tap in two parts, so that a row loop hoists the first.  The row `dy` pixels from y: whether it lies in the image, and the first address of a legal
// row (outside: the pixel's own) ...
struct ImgRow
{
    bool in;
    uint32_t base;
};
SKH_DI ImgRow img_row(uint32_t y, int dy, uint32_t width, int H)
{
    const int qy = (int)y + dy;
    ImgRow r;
    r.in = qy >= 0 && qy < H;
    r.base = (uint32_t)(r.in ? qy : (int)y) * width;
    return r;
}
// ... and the tap `dx` pixels from x in it: whether it lies in the image, and the address j to load (a tap outside reads the row's centre column: a legal
// address, a value never used)
SKH_DI bool img_tap(const ImgRow& r, uint32_t x, int dx, int W, uint32_t& j)
{
    const int qx = (int)x + dx;
    const bool in = r.in && qx >= 0 && qx < W;
    j = r.base + (uint32_t)(in ? qx : (int)x);
    return in;
}

// Where the pixel (x, y) with the first-hit position P lay in the previous frame: the projection (fx, fy) through prevWorldToClip and whether it lands on the
// image's bilinear support; the four taps around it -- their weights and the first tap's pixel.  A pixel that does not project gathers around itself: legal,
// never used.  (A tap's address is worked out where it is loaded, img_footprint_tap, not here for all four: ahead of the sixteen loads of k_tp_reproject the four
// addresses cost that kernel two registers.)
struct ImgFootprint
{
    bool projects;
    float fx, fy;
    float w[4];
    int qx0, qy0; // the first tap: -1 .. W, -1 .. H
};
SKH_DI ImgFootprint img_footprint(const float* prevWorldToClip, uint32_t width, uint32_t height, const float4& P, uint32_t x, uint32_t y)
{
    ImgFootprint f;
    const float W = (float)width, H = (float)height; // (exact: <= 2^26)
    const v4 clip = mul44(prevWorldToClip, mk4(P.x, P.y, P.z, 1.0f));
    f.fx = ((clip.x / clip.w) * 0.5f + 0.5f) * W - 0.5f;
    f.fy = ((clip.y / clip.w) * 0.5f + 0.5f) * H - 0.5f;
    // (every comparison false for a NaN; the range test before the conversion to an integer)
    f.projects = clip.w > 0.0f && dn_finite(f.fx) && dn_finite(f.fy) && f.fx >= -1.0f && f.fx <= W && f.fy >= -1.0f && f.fy <= H;
    const float gx = f.projects ? f.fx : (float)x, gy = f.projects ? f.fy : (float)y;
    const float flx = floorf(gx), fly = floorf(gy);
    f.qx0 = (int)flx, f.qy0 = (int)fly;
    const float tx = gx - flx, ty = gy - fly;
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    f.w[0] = ux * uy, f.w[1] = tx * uy, f.w[2] = ux * ty, f.w[3] = tx * ty;
    return f;
}
// tap k of the footprint (k & 1: one pixel to the right, k >> 1: one down): whether it lies in the image, and its address j clamped into it
SKH_DI bool img_footprint_tap(const ImgFootprint& f, int k, uint32_t width, uint32_t height, uint32_t& j)
{
    const int Wi = (int)width, Hi = (int)height;
    const int qx = f.qx0 + (k & 1), qy = f.qy0 + (k >> 1);
    const int ax = qx < 0 ? 0 : (qx < Wi ? qx : Wi - 1), ay = qy < 0 ? 0 : (qy < Hi ? qy : Hi - 1);
    j = (uint32_t)ay * width + (uint32_t)ax;
    return qx >= 0 && qx < Wi && qy >= 0 && qy < Hi;
}

// the normal and the plane term of a filter tap (gq, pq) seen from the centre (gp, pp), in the packed guide record {N.xyz, P.x}, {P.y, P.z}
SKH_DI void img_guides(const float4& gp, const float2& pp, const float4& gq, const float2& pq, float kn, float kp, float& tn, float& tp)
{
    const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
    tn = ((nx * nx + ny * ny) + nz * nz) * kn;
    const float px = gq.w - gp.w, py = pq.x - pp.x, pz = pq.y - pp.y;
    const float d = (gp.x * px + gp.y * py) + gp.z * pz;
    tp = (d * d) * kp;
}

// One pass over the caller's images -> per pixel a 16-byte colour record and a 24-byte guide record {N.xyz, P.x}, {P.y, P.z}: a filter tap costs 40 bytes instead
// of 80 and never looks at IDS again.  Every word is a copy of a float32 of the definition: the packing is lossless.  The colour record's fourth word marks the
// surface pixels.  Without VARIANCE: 1 on a surface pixel, 0 on every other.  With it: the variance moments[i].z, >= 0, on a surface pixel and -1 on every other.
// One lane, one pixel, a one-dimensional launch of 256-lane blocks; `demodulate`: the colour is divided by the floored albedo; `moments` is read with VARIANCE only.
template <bool VARIANCE>
__global__ void __launch_bounds__(256) k_img_pack(uint32_t pixels, uint32_t demodulate, float albedoFloor, const float4* __restrict__ color,
                                                   const uint4* __restrict__ ids, const float4* __restrict__ normal, const float4* __restrict__ position,
                                                   const float4* __restrict__ albedo, const float4* __restrict__ moments, float4* __restrict__ c0,
                                                   float4* __restrict__ g0, float2* __restrict__ g1)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels)
        return;
    const float4 c = color[i];
    float4 rc = make_float4(0.0f, 0.0f, 0.0f, VARIANCE ? -1.0f : 0.0f), rg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 rp = make_float2(0.0f, 0.0f);
    if (img_surface(ids[i].w, c.x, c.y, c.z))
    {
        float m = 1.0f;
        if (VARIANCE)
        {
            const float z = moments[i].z;
            m = (dn_finite(z) && z > 0.0f) ? z : 0.0f;
        }
        rc = make_float4(c.x, c.y, c.z, m);
        if (demodulate)
        {
            const float3 a = img_albedo(albedo[i], albedoFloor);
            rc.x = c.x / a.x, rc.y = c.y / a.y, rc.z = c.z / a.z;
        }
        const float4 n = normal[i], p = position[i];
        rg = make_float4(n.x, n.y, n.z, p.x);
        rp = make_float2(p.y, p.z);
    }
    c0[i] = rc;
    g0[i] = rg;
    g1[i] = rp;
}

} // namespace skh
