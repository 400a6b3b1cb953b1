// strelka_hip -- sampling tables of the environment light (the device functions that read them: skh_device.h, env_eval / env_sample).
//
//   k_env_rows       one workgroup per row: the texel weights w = luminance_709 * sin(pi (iy + 1/2) / H), the row's inclusive scan
//                    (wave scan by __shfl_up, the four wave totals through LDS), its conditional CDF and its sum
//   k_env_marginal   one workgroup: the scan of the H <= 4096 row sums -> marginal CDF, sum w
//   k_env_normalise  w -> w / sum w in the texels' fourth word
//
// A weight is computed in double and kept as one float per texel; every sum over those floats is a double.  A sun texel 10^6 times its
// neighbours therefore takes nothing away from them, and a stored CDF value is one rounding away from the exact CDF of the stored weights.
#pragma once
#include "skh_device.h"

namespace skh
{

#define SKH_ENV_MAX_WIDTH 8192u
#define SKH_ENV_MAX_HEIGHT 4096u
#define SKH_ENV_BLOCK 256u

// exclusive scan of one double per thread over the 256-thread workgroup; total = the workgroup's sum (s_part: one double per wave, used once per kernel)
SKH_DI double env_block_scan(double v, double* s_part, double& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        const double t = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o)
            inc += t;
    }
    const double before = __shfl_up(inc, 1, 64);
    if (lane == 63u)
        s_part[wave] = inc;
    __syncthreads();
    double base = 0.0;
    total = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < SKH_ENV_BLOCK / 64u; ++k)
    {
        if (k < wave)
            base += s_part[k];
        total += s_part[k];
    }
    return base + (lane ? before : 0.0);
}

// Thread t owns the `per` consecutive entries from t * per on (per <= 32 for a row of 8192): inclusive scan of s_v[0..n) in place, normalised by the
// total -> a CDF; the uniform CDF when the total is 0 (such a row is never selected; an all-black map is legal), so that every entry is a number.
SKH_DI double env_scan_to_cdf(float* s_v, uint32_t n, double* s_part)
{
    const uint32_t per = (n + SKH_ENV_BLOCK - 1u) / SKH_ENV_BLOCK;
    const uint32_t first = min(threadIdx.x * per, n), last = min(first + per, n);
    double mine = 0.0;
    for (uint32_t i = first; i < last; ++i)
        mine += (double)s_v[i];
    double total;
    double run = env_block_scan(mine, s_part, total);
    for (uint32_t i = first; i < last; ++i)
    {
        run += (double)s_v[i];
        s_v[i] = total > 0.0 ? (float)(run / total) : (float)(i + 1u) / (float)n;
    }
    return total;
}

// rgb: W x H x 3 floats as the caller gave them.  texels: {r, g, b, w} (w not yet normalised).  *bad is set when a value is negative or not finite.
__global__ void __launch_bounds__(SKH_ENV_BLOCK) k_env_rows(const float* __restrict__ rgb, uint32_t W, uint32_t H, float4* __restrict__ texels,
                                                             float* __restrict__ colCdf, double* __restrict__ rowSum, uint32_t* __restrict__ bad)
{
    __shared__ float s_w[SKH_ENV_MAX_WIDTH];
    __shared__ double s_part[SKH_ENV_BLOCK / 64u];
    const uint32_t iy = blockIdx.x;
    if (iy >= H || W > SKH_ENV_MAX_WIDTH) // (the whole workgroup: no barrier is left behind)
        return;
    const double sinRow = sin(3.14159265358979323846 * ((double)iy + 0.5) / (double)H);
    const size_t row0 = (size_t)iy * W;
    bool anyBad = false;
    for (uint32_t ix = threadIdx.x; ix < W; ix += SKH_ENV_BLOCK)
    {
        const float* p = rgb + 3u * (row0 + ix);
        const float r = p[0], g = p[1], b = p[2];
        anyBad = anyBad || !(r >= 0.0f && g >= 0.0f && b >= 0.0f) || isinf(r) || isinf(g) || isinf(b); // (a NaN fails >=)
        const float w = (float)((0.2126 * (double)r + 0.7152 * (double)g + 0.0722 * (double)b) * sinRow);
        s_w[ix] = w;
        texels[row0 + ix] = make_float4(r, g, b, w);
    }
    if (anyBad)
        atomicOr(bad, 1u);
    __syncthreads();
    const double total = env_scan_to_cdf(s_w, W, s_part);
    __syncthreads();
    for (uint32_t ix = threadIdx.x; ix < W; ix += SKH_ENV_BLOCK)
        colCdf[row0 + ix] = s_w[ix];
    if (threadIdx.x == 0)
        rowSum[iy] = total;
}

// one workgroup; the row sums stay doubles (env_scan_to_cdf's float staging would round them)
__global__ void __launch_bounds__(SKH_ENV_BLOCK) k_env_marginal(const double* __restrict__ rowSum, uint32_t H, float* __restrict__ rowCdf, double* __restrict__ sumW)
{
    __shared__ double s_part[SKH_ENV_BLOCK / 64u];
    const uint32_t per = (H + SKH_ENV_BLOCK - 1u) / SKH_ENV_BLOCK;
    const uint32_t first = min(threadIdx.x * per, H), last = min(first + per, H);
    double mine = 0.0;
    for (uint32_t i = first; i < last; ++i)
        mine += rowSum[i];
    double total;
    double run = env_block_scan(mine, s_part, total);
    for (uint32_t i = first; i < last; ++i)
    {
        run += rowSum[i];
        rowCdf[i] = total > 0.0 ? (float)(run / total) : (float)(i + 1u) / (float)H;
    }
    if (threadIdx.x == 0)
        *sumW = total;
}

__global__ void __launch_bounds__(SKH_ENV_BLOCK) k_env_normalise(float4* __restrict__ texels, size_t n, const double* __restrict__ sumW)
{
    const double total = *sumW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        texels[i].w = total > 0.0 ? (float)((double)texels[i].w / total) : 0.0f;
}

// SKH_UNIT_ENV_SAMPLE (u[2] -> dir[3], pdf, Le[3], ix, iy) and SKH_UNIT_ENV_EVAL (dir[3] -> Le[3], pdf, ix, iy): the functions k_shade calls
__global__ void __launch_bounds__(256) k_env_probe(EnvP env, uint32_t sample, const float* __restrict__ in, uint32_t n, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    v3 dir;
    EnvEval ev;
    uint32_t ix, iy;
    if (sample)
    {
        const EnvSample s = env_sample(env, in[2 * (size_t)i], in[2 * (size_t)i + 1]);
        dir = s.dir, ev = s.ev, ix = s.ix, iy = s.iy;
        uint32_t* o = out + 9 * (size_t)i;
        o[0] = __float_as_uint(dir.x), o[1] = __float_as_uint(dir.y), o[2] = __float_as_uint(dir.z), o[3] = __float_as_uint(ev.pdf);
        o[4] = __float_as_uint(ev.Le.x), o[5] = __float_as_uint(ev.Le.y), o[6] = __float_as_uint(ev.Le.z), o[7] = ix, o[8] = iy;
    }
    else
    {
        ev = env_eval(env, mk3(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]));
        uint32_t* o = out + 6 * (size_t)i;
        o[0] = __float_as_uint(ev.Le.x), o[1] = __float_as_uint(ev.Le.y), o[2] = __float_as_uint(ev.Le.z), o[3] = __float_as_uint(ev.pdf), o[4] = ev.ix, o[5] = ev.iy;
    }
}

} // namespace skh
