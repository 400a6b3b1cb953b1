// strelka_hip -- the emitter table of emissive meshes (the device functions that read it: skh_device.h, emit_select / emit_sample / emit_pdf).
//
//   k_emit_gather     one thread per entry = (emitting mesh instance, triangle of its mesh): the world-space vertices through the instance transform, the world area,
//                     the weight w = area * luminance_709(Le) -> the 64-byte entry and one float of weight
//   k_emit_tile_sums  one workgroup per tile of SKH_EMIT_TILE weights: the tile's sum, in double
//   k_emit_scan_tiles one workgroup: exclusive scan of the tile sums (<= 2^24 / 2048 = 8192 of them) -> tile bases, sum w
//   k_emit_cdf        one workgroup per tile again: its inclusive scan on top of its base, divided by sum w -> the CDF
//   k_emit_guide      one thread per guide bucket: the entry the search returns for u = b / G
//
// A weight is computed in float from float vertices and kept as one float per entry; every sum over those floats is a double (a device-wide scan in three passes,
// any number of workgroups): a stored CDF value is one rounding away from the exact CDF of the stored weights, as skh_env.h promises for its tables.
#pragma once
#include "skh_env.h"

namespace skh
{

#define SKH_EMIT_BLOCK 256u // (= SKH_ENV_BLOCK: env_block_scan is the workgroup scan of both)
#define SKH_EMIT_PER 8u // consecutive entries per thread
#define SKH_EMIT_TILE (SKH_EMIT_BLOCK * SKH_EMIT_PER)
static_assert(SKH_EMIT_BLOCK == SKH_ENV_BLOCK, "env_block_scan scans SKH_ENV_BLOCK threads");

// emitInst: the emitting instances, emitBase[j] = first entry of the j-th of them (nEmitInst + 1 values, the last one = nEntries).  instances: the uploaded skh_instance table.
__global__ void __launch_bounds__(SKH_EMIT_BLOCK) k_emit_gather(const uint8_t* __restrict__ verts, const uint32_t* __restrict__ indices, const uint4* __restrict__ meshes,
                                                                const uint32_t* __restrict__ instances /* skh_instance: 16 words */, const float4* __restrict__ Le, uint32_t numMaterials,
                                                                const uint32_t* __restrict__ emitInst, const uint32_t* __restrict__ emitBase, uint32_t nEmitInst,
                                                                uint32_t nEntries, float4* __restrict__ entries, float* __restrict__ weight)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nEntries)
        return;
    uint32_t lo = 0, hi = nEmitInst; // emitBase[lo] <= g < emitBase[hi]
    while (hi - lo > 1u)
    {
        const uint32_t mid = (lo + hi) >> 1;
        if (emitBase[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t inst = emitInst[lo], prim = g - emitBase[lo];
    const uint4* ip = reinterpret_cast<const uint4*>(instances) + 4 * (size_t)inst; // {o2w[12] | type, geom, material, light}
    const uint4 r0 = ip[0], r1 = ip[1], r2 = ip[2], ids = ip[3];
    const float m[12] = { __uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w), __uint_as_float(r1.x), __uint_as_float(r1.y),
                          __uint_as_float(r1.z), __uint_as_float(r1.w), __uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z), __uint_as_float(r2.w) };
    const uint4 me = meshes[ids.y];
    v3 w[3];
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
    {
        const uint32_t idx = indices[me.x + 3u * prim + k];
        const float* v = reinterpret_cast<const float*>(verts + (size_t)(me.z + idx) * 32);
        w[k] = xform_point(m, mk3(v[0], v[1], v[2]));
    }
    const float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
    const uint32_t mid0 = ids.z == 0xffffffffu ? 0u : ids.z; // (as k_shade reads it)
    const float4 le = Le[mid0 < numMaterials ? mid0 : 0u];
    const float area = 0.5f * length(cross(w[1] - w[0], w[2] - w[0]));
    float wk = area * le.w;
    if (!(wk > 0.0f) || isinf(wk)) // (a degenerate triangle, vertices that are not numbers)
        wk = 0.0f;
    float4* o = entries + 4 * (size_t)g;
    o[0] = make_float4(w[0].x, w[0].y, w[0].z, le.x);
    o[1] = make_float4(w[1].x, w[1].y, w[1].z, le.y);
    o[2] = make_float4(w[2].x, w[2].y, w[2].z, le.z);
    o[3] = make_float4(le.w, __uint_as_float(inst), __uint_as_float(prim | (det < 0.0f ? 0x80000000u : 0u)), 0.0f);
    weight[g] = wk;
}

// the thread's SKH_EMIT_PER consecutive weights of tile blockIdx.x (0 past the end) and their sum
SKH_DI double emit_load_run(const float* __restrict__ weight, uint32_t n, float* w)
{
    const size_t first = (size_t)blockIdx.x * SKH_EMIT_TILE + (size_t)threadIdx.x * SKH_EMIT_PER;
    double mine = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < SKH_EMIT_PER; ++k)
    {
        w[k] = first + k < n ? weight[first + k] : 0.0f;
        mine += (double)w[k];
    }
    return mine;
}

__global__ void __launch_bounds__(SKH_EMIT_BLOCK) k_emit_tile_sums(const float* __restrict__ weight, uint32_t n, double* __restrict__ tileSum)
{
    __shared__ double s_part[SKH_EMIT_BLOCK / 64u];
    float w[SKH_EMIT_PER];
    const double mine = emit_load_run(weight, n, w);
    double total;
    (void)env_block_scan(mine, s_part, total);
    if (threadIdx.x == 0)
        tileSum[blockIdx.x] = total;
}

// one workgroup: tileSum -> the sum of the tiles before each one, in place; *sumW = the sum of all
__global__ void __launch_bounds__(SKH_EMIT_BLOCK) k_emit_scan_tiles(double* __restrict__ tileSum, uint32_t nTiles, double* __restrict__ sumW)
{
    __shared__ double s_part[SKH_EMIT_BLOCK / 64u];
    const uint32_t per = (nTiles + SKH_EMIT_BLOCK - 1u) / SKH_EMIT_BLOCK;
    const uint32_t first = min(threadIdx.x * per, nTiles), last = min(first + per, nTiles);
    double mine = 0.0;
    for (uint32_t i = first; i < last; ++i)
        mine += tileSum[i];
    double total;
    double run = env_block_scan(mine, s_part, total);
    for (uint32_t i = first; i < last; ++i)
    {
        const double t = tileSum[i];
        tileSum[i] = run;
        run += t;
    }
    if (threadIdx.x == 0)
        *sumW = total;
}

__global__ void __launch_bounds__(SKH_EMIT_BLOCK) k_emit_cdf(const float* __restrict__ weight, uint32_t n, const double* __restrict__ tileBase,
                                                             const double* __restrict__ sumW, float* __restrict__ cdf)
{
    __shared__ double s_part[SKH_EMIT_BLOCK / 64u];
    float w[SKH_EMIT_PER];
    const double mine = emit_load_run(weight, n, w);
    double tileTotal;
    double run = tileBase[blockIdx.x] + env_block_scan(mine, s_part, tileTotal);
    const double total = *sumW;
    const size_t first = (size_t)blockIdx.x * SKH_EMIT_TILE + (size_t)threadIdx.x * SKH_EMIT_PER;
#pragma unroll
    for (uint32_t k = 0; k < SKH_EMIT_PER; ++k)
        if (first + k < n)
        {
            run += (double)w[k];
            cdf[first + k] = total > 0.0 ? (float)(run / total) : (float)(first + k + 1u) / (float)n; // (sum w = 0: never sampled; every entry a number)
        }
}

// guide[b] = smallest i with b / G < cdf[i], at most n - 1, for b < G = 2^bits; guide[G] = n - 1
__global__ void __launch_bounds__(SKH_EMIT_BLOCK) k_emit_guide(const float* __restrict__ cdf, uint32_t n, uint32_t bits, uint32_t* __restrict__ guide)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x, G = 1u << bits;
    if (b > G)
        return;
    uint32_t lo = 0u, hi = n - 1u;
    if (b < G)
    {
        const float u = (float)b / (float)G; // exact: G is a power of two <= 2^24
        while (lo < hi)
        {
            const uint32_t mid = (lo + hi) >> 1;
            if (u < cdf[mid])
                hi = mid;
            else
                lo = mid + 1u;
        }
    }
    else
        lo = hi;
    guide[b] = lo;
}

// skh_emitter_probe: SKH_EMIT_PROBE_SAMPLE ({u', ux, uy, P[3]} -> 13 words) and SKH_EMIT_PROBE_PDF ({instance, prim, hitPoint[3], origin[3]} -> 4 words)
__global__ void __launch_bounds__(256) k_emit_probe(EmitP em, uint32_t numInstances, uint32_t kind, const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    if (kind == 0u)
    {
        const float* q = reinterpret_cast<const float*>(in) + 6 * (size_t)i;
        const EmitSample s = emit_sample(em, q[0], q[1], q[2], mk3(q[3], q[4], q[5]));
        uint32_t* o = out + 13 * (size_t)i;
        o[0] = __float_as_uint(s.point.x), o[1] = __float_as_uint(s.point.y), o[2] = __float_as_uint(s.point.z);
        o[3] = __float_as_uint(s.normal.x), o[4] = __float_as_uint(s.normal.y), o[5] = __float_as_uint(s.normal.z);
        o[6] = __float_as_uint(s.Le.x), o[7] = __float_as_uint(s.Le.y), o[8] = __float_as_uint(s.Le.z);
        o[9] = __float_as_uint(s.pdf), o[10] = __float_as_uint(s.dist), o[11] = s.instance, o[12] = s.prim;
    }
    else
    {
        const uint32_t* q = in + 8 * (size_t)i;
        const uint32_t inst = q[0], prim = q[1];
        uint32_t* o = out + 4 * (size_t)i;
        o[0] = o[1] = o[2] = o[3] = 0u;
        const uint32_t base = inst < numInstances ? em.instOffset[inst] : 0xffffffffu;
        if (base == 0xffffffffu)
            return;
        const uint32_t end = em.count; // (the instance's entries end where the next emitter's begin: an entry names its instance)
        if (prim >= end - base)
            return;
        const float4* p = em.entries + 4 * (size_t)(base + prim);
        const float4 a = p[0], b = p[1], c = p[2], d = p[3];
        if (__float_as_uint(d.y) != inst)
            return;
        const v3 ne = emit_normal(mk3(a), mk3(b), mk3(c), (__float_as_uint(d.z) >> 31) != 0u);
        const float pdf = emit_pdf(ne, d.x * em.invSumW, mk3(__uint_as_float(q[2]), __uint_as_float(q[3]), __uint_as_float(q[4])),
                                   mk3(__uint_as_float(q[5]), __uint_as_float(q[6]), __uint_as_float(q[7])));
        o[0] = __float_as_uint(pdf), o[1] = __float_as_uint(a.w), o[2] = __float_as_uint(b.w), o[3] = __float_as_uint(c.w);
    }
}

} // namespace skh
