// strelka_hip -- adaptive sampling (skh_set_adaptive; DESIGN.md section 2 "Adaptive sampling"): per-pixel statistics of the observations the accumulator
// receives, the per-tile decision, and the copy of frozen tiles into the caller's image.
//
// Included at the end of skh_kernels.h: these kernels read what the accumulation kernels read (FrameP, PathS, the sums of k_collect) and share slot_to_pixel.
// They run only in a context with the feature on; k_finalize / k_finalize_batch and everything before them are not touched.
//
// State: one float4 per slot {n, mean, M2, q at the tile's last check}.  All three kernels are bound by memory: k_adapt_moments reads and writes the 16 bytes
// of state once per pixel and launch (plus the radiances k_finalize_batch has just read: 16 B per sub-frame of the pass), k_adapt_tiles reads them once per
// check and writes q, k_adapt_fill moves 16 B per pixel of a frozen tile and call.  No scratch, no atomics.
#pragma once

namespace skh
{

#define SKH_ADAPT_OFF 0x40000000u // origin of a frozen tile in the render list: off every image (slot_to_pixel fails), and origin + T does not wrap

// LDR luminance of one observation: products and sums rounded one by one, left to right (the library is built without contraction)
SKH_DI float adapt_luma(const v3& result, const v3& exposure)
{
    const v3 t = tonemap(result, exposure);
    return 0.2126f * t.x + 0.7152f * t.y + 0.0722f * t.z;
}
// Welford's update of {n, mean, M2} in s.x, s.y, s.z
SKH_DI void adapt_fold(float4& s, float y)
{
    s.x += 1.0f;
    const float d = y - s.y;
    s.y += d / s.x;
    s.z += d * (y - s.y);
}
// a maximum that keeps a NaN from either side
SKH_DI float adapt_nanmax(float a, float b)
{
    return (a > b || a != a) ? a : b;
}

// Folds the observations of one pass into the state, in sub-frame order: sub-frames [finalFirst, finalFirst + finalCount) of a batched pass (one sample each, read
// from the path state as k_finalize_batch reads them), or the one launch of fp.samplesThisLaunch samples whose sums k_collect left (fromSums).  `tileXY` is
// the RENDER list: slots of frozen tiles fail slot_to_pixel like slots outside the image.
__global__ void __launch_bounds__(256)
    k_adapt_moments(FrameP fp, const uint32_t* __restrict__ tileXY, PathS ps, const float* __restrict__ sums, uint32_t fromSums, float4* __restrict__ state)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t px, py;
    if (slot >= fp.numSlots || !slot_to_pixel(fp, tileXY, slot, px, py))
        return;
    const v3 exposure = mk3(fp.exposure[0], fp.exposure[1], fp.exposure[2]);
    float4 s = state[slot];
    if (fromSums)
    {
        const size_t N = fp.numSlots;
        const v3 result = mk3(sums[slot], sums[slot + N], sums[slot + 2 * N]) / (float)fp.samplesThisLaunch;
        adapt_fold(s, adapt_luma(result, exposure));
    }
    else
        for (uint32_t sub = fp.finalFirst; sub < fp.finalFirst + fp.finalCount; ++sub)
        {
            const v3 result = (mk3(0.0f) + mk3(ps.rad()[(size_t)sub * fp.numSlots + slot])) / 1.0f; // (k_finalize_batch, finalize_one)
            adapt_fold(s, adapt_luma(result, exposure));
        }
    state[slot] = s;
}

// One check: one workgroup per tile.  q per valid pixel into the state's fourth word; Q = max q over the tile, through the wave's lanes and then through LDS; the
// tile freezes iff Q <= thr2 -- then its observation count goes into frozenAt[tile] (0 = active) and its origin in the render list moves off the image.
// A tile frozen at an earlier check is left as it is.
__global__ void __launch_bounds__(256) k_adapt_tiles(FrameP fp, uint32_t* __restrict__ renderXY, float4* __restrict__ state, uint32_t n, float thr2,
                                                     float darkLevel, float* __restrict__ tileQ, uint32_t* __restrict__ frozenAt)
{
    __shared__ float s_q[4];
    const uint32_t tile = blockIdx.x;
    if (tile >= fp.numTiles || frozenAt[tile] != 0u) // (uniform over the workgroup)
        return;
    const uint32_t T2 = 1u << (2 * fp.tileShift);
    float qmax = 0.0f; // (q >= 0 or NaN)
    for (uint32_t m = threadIdx.x; m < T2; m += blockDim.x)
    {
        const uint32_t slot = tile * T2 + m;
        uint32_t px, py;
        if (!slot_to_pixel(fp, renderXY, slot, px, py))
            continue;
        float4 s = state[slot];
        const float v = s.z / s.x, e2 = v / s.x;
        const float ref = s.y > darkLevel ? s.y : darkLevel;
        const float q = e2 / (ref * ref);
        s.w = q;
        state[slot] = s;
        qmax = adapt_nanmax(qmax, q);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        qmax = adapt_nanmax(qmax, __shfl_xor(qmax, off, 64));
    if ((threadIdx.x & 63u) == 0u)
        s_q[threadIdx.x >> 6] = qmax;
    __syncthreads(); // (also: every lane has read the tile's origin before thread 0 moves it)
    if (threadIdx.x == 0)
    {
        float Q = s_q[0];
        for (uint32_t w = 1; w < (blockDim.x >> 6); ++w)
            Q = adapt_nanmax(Q, s_q[w]);
        tileQ[tile] = Q;
        if (Q <= thr2)
        {
            frozenAt[tile] = n;
            renderXY[2 * tile] = SKH_ADAPT_OFF;
            renderXY[2 * tile + 1] = SKH_ADAPT_OFF;
        }
    }
}

// A call's d_image holds the whole owned image: the accumulation kernels write the pixels of the active tiles, this one the pixels of the frozen ones (what
// the accumulation step wrote there when the tile was last traced: the accumulator itself).  homeXY: the context's tile list, where every tile is.
__global__ void __launch_bounds__(256) k_adapt_fill(FrameP fp, const uint32_t* __restrict__ homeXY, const uint32_t* __restrict__ frozenAt,
                                                    const float4* __restrict__ accum, float4* __restrict__ image)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t px, py;
    if (slot >= fp.numSlots || frozenAt[slot >> (2 * fp.tileShift)] == 0u || !slot_to_pixel(fp, homeXY, slot, px, py))
        return;
    image[(size_t)py * fp.width + px] = accum[slot];
}

} // namespace skh
