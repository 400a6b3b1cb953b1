// strelka_hip -- host side of the C ABI declared in include/strelka_hip.h (gfx950 / ROCm only).
// One translation unit: device code comes from skh_device.h / skh_bvh.h / skh_kernels.h.
#include "../../include/strelka_hip.h"
#include "skh_kernels.h"

#include <dlfcn.h>
// RCCL is dlopen()ed on first use (skh_comm_*); the handful of types its point-to-point API needs are declared here, so that a
// box without the RCCL development headers still builds the renderer (nccl.h 2.x: the layouts below are part of its stable ABI)
typedef struct ncclComm* ncclComm_t;
typedef struct
{
    char internal[128];
} ncclUniqueId;
typedef enum
{
    ncclSuccess = 0
} ncclResult_t;
typedef enum
{
    ncclFloat = 7 // ncclFloat32
} ncclDataType_t;

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace skh;

static_assert(sizeof(skh_vertex) == 32 && sizeof(skh_instance) == 64 && sizeof(skh_light) == 112, "ABI layout");
static_assert(sizeof(skh_material) == 64 && sizeof(skh_frame_params) == 176 && sizeof(skh_ray) == 32, "ABI layout");
static_assert(sizeof(skh_hit) == 20 && sizeof(Light) == 112 && sizeof(Material) == 64 && sizeof(HostInstance) == 64, "layout");

#include "skh_host.h"
#include "skh_aov.h"
#include "skh_image.h"
#include "skh_denoise.h"
#include "skh_temporal.h"
#include "skh_variance.h"
#include "skh_motion.h"
#include "skh_rectify.h"


// Sobol generator matrices for the 5 dimensions the reference tabulates (RandomSampler.h:139-164), produced from the
// Joe-Kuo recurrences (d=2: s=1 a=0 m={1}; d=3: s=2 a=1 m={1,3}; d=4: s=3 a=1 m={1,3,1}; d=5: s=3 a=2 m={1,1,1}).
static void init_sobol_table(uint32_t tab[5][32])
{
    for (int i = 0; i < 32; ++i)
        tab[0][i] = 1u << (31 - i);
    const int S[4] = { 1, 2, 3, 3 };
    const uint32_t A[4] = { 0, 1, 1, 2 };
    const uint32_t M[4][3] = { { 1, 0, 0 }, { 1, 3, 0 }, { 1, 3, 1 }, { 1, 1, 1 } };
    for (int d = 0; d < 4; ++d)
    {
        uint32_t* v = tab[d + 1];
        const int s = S[d];
        for (int i = 0; i < s; ++i)
            v[i] = M[d][i] << (31 - i);
        for (int i = s; i < 32; ++i)
        {
            uint32_t x = v[i - s] ^ (v[i - s] >> s);
            for (int k = 1; k < s; ++k)
                if ((A[d] >> (s - 1 - k)) & 1u)
                    x ^= v[i - k];
            v[i] = x;
        }
    }
}


// The entry points below take C linkage from their declarations in include/strelka_hip.h.

// Ends the speculation.  Whatever was traced ahead and not yet delivered is dropped: its share of the pass's rays (sub-frames of a
// pass trace the same pixels with different samples: equal shares to a fraction of a per cent) leaves the ray counts.
// A drop that forgets the previous call as well (keepLast = false) is what every scene setter, skh_resize and skh_set_tiles do first: there the adaptive frame
// starts again too (all tiles active, statistics cleared: adapt_prepare at the next adaptive call) -- unless the caller is a render entry point (keepAdaptive).
static void spec_drop(skh_context* c, bool keepLast = false, bool keepAdaptive = false)
{
    skh_context::Speculation& sp = c->spec;
    if (!keepLast && !keepAdaptive)
        c->adapt.ready = false;
    if (sp.nextInFlight)
    {
        // a whole pass traced ahead that nobody will collect: wait for it (its buffers are about to be reused), take its rays out again
        unsigned long long after[2] = { 0, 0 };
        (void)hipStreamSynchronize(c->dev.stream);
        if (hipMemcpy(after, c->timing.dStats.p, sizeof(after), hipMemcpyDeviceToHost) == hipSuccess)
        {
            c->spec.discardedRadiance += after[0] - sp.statsMark[0];
            c->spec.discardedShadow += after[1] - sp.statsMark[1];
        }
        c->spec.discardedSubframes += sp.nextCount;
        sp.nextInFlight = false;
    }
    if (sp.valid && sp.consumed < sp.count && sp.count > 0)
    {
        const uint32_t left = sp.count - sp.consumed;
        c->spec.discardedRadiance += sp.passRadiance * left / sp.count;
        c->spec.discardedShadow += sp.passShadow * left / sp.count;
        c->spec.discardedSubframes += left;
    }
    sp.valid = false;
    sp.buf = 0;
    if (!keepLast)
        sp.haveLast = false;
}

// Where work on what an earlier pass delivered runs (accumulation steps, tone mapping, image copies): beside a pass traced ahead, not behind it.
static inline hipStream_t side_stream(const skh_context* c)
{
    return c->spec.nextInFlight ? c->dev.stream3 : c->dev.stream;
}

uint32_t skh_abi_version(void)
{
    return SKH_ABI_VERSION;
}

skh_status skh_create(int device_ordinal, skh_context** out_ctx)
{
    if (!out_ctx)
        return SKH_INVALID_ARGUMENT;
    *out_ctx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_ordinal < 0 || device_ordinal >= count)
        return SKH_FAIL; // no GPU: the product path fails loudly, there is no CPU fallback
    skh_context* c = new skh_context();
    c->dev.device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess || hipStreamCreate(&c->dev.stream) != hipSuccess || hipStreamCreate(&c->dev.stream2) != hipSuccess || hipStreamCreateWithFlags(&c->dev.stream3, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->dev.evShade, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->dev.evShadow, hipEventDisableTiming) != hipSuccess)
    {
        delete c;
        return SKH_FAIL;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess)
        c->dev.numCUs = prop.multiProcessorCount;
    uint32_t tab[5][32];
    init_sobol_table(tab);
    std::vector<uint32_t> lut(SKH_SOBOL_LUT_WORDS);
    for (uint32_t d = 0; d < 5; ++d)
        for (uint32_t b = 0; b < 4; ++b)
            for (uint32_t v = 0; v < 256; ++v)
            {
                uint32_t x = 0;
                for (uint32_t j = 0; j < 8; ++j)
                    if ((v >> j) & 1u)
                        x ^= tab[d][8 * b + j];
                lut[(d * 4 + b) * 256 + v] = x;
            }
    if (hipMemcpyToSymbol(HIP_SYMBOL(c_sobol), tab, sizeof(tab)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_sobol_lut), lut.data(), lut.size() * sizeof(uint32_t)) != hipSuccess)
    {
        delete c;
        return SKH_FAIL;
    }
    if (dev_alloc(c, c->timing.dStats, sizeof(StatsDev)) != SKH_OK || hipMemset(c->timing.dStats.p, 0, sizeof(StatsDev)) != hipSuccess ||
        dev_alloc(c, c->cut.dStats, sizeof(CutStatsDev)) != SKH_OK || hipMemset(c->cut.dStats.p, 0, sizeof(CutStatsDev)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->dev.hOverflow), 64, hipHostMallocMapped) != hipSuccess)
    {
        delete c;
        return SKH_FAIL;
    }
    *c->dev.hOverflow = 0u;
    *out_ctx = c;
    return SKH_OK;
}

void skh_destroy(skh_context* c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->dev.device);
    (void)hipStreamSynchronize(c->dev.stream);
    if (c->dev.stream3)
        (void)hipStreamSynchronize(c->dev.stream3);
    if (c->multi.comm)
        (void)skh_comm_destroy(c);
    for (hipEvent_t e : c->timing.eventPool)
        (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->dev.stream);
    if (c->dev.stream2)
        (void)hipStreamDestroy(c->dev.stream2);
    if (c->dev.stream3)
        (void)hipStreamDestroy(c->dev.stream3);
    if (c->dev.evShade)
        (void)hipEventDestroy(c->dev.evShade);
    if (c->dev.evShadow)
        (void)hipEventDestroy(c->dev.evShadow);
    if (c->dev.hOverflow)
        (void)hipHostFree(c->dev.hOverflow);
    delete c; // (frees every device buffer the context owns)
}

const char* skh_last_error(const skh_context* c)
{
    return c ? c->dev.err.c_str() : "null context";
}

// FNV-1a over 32-bit words, continued from h: the topology signatures of skh_set_geometry and skh_set_curves
static const uint64_t kFnv1aSeed = 1469598103934665603ull;
static uint64_t fnv1a_words(uint64_t h, const void* words, size_t n)
{
    const uint32_t* w = static_cast<const uint32_t*>(words);
    for (size_t k = 0; k < n; ++k)
        h = (h ^ w[k]) * 1099511628211ull;
    return h;
}

skh_status skh_set_geometry(skh_context* c, const skh_vertex* verts, uint32_t n_verts, const uint32_t* indices, uint32_t n_indices,
                            const skh_mesh* meshes, uint32_t n_meshes)
{
    if (!c || (n_verts && !verts) || (n_indices && !indices) || (n_meshes && !meshes))
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    for (uint32_t m = 0; m < n_meshes; ++m)
    {
        const skh_mesh& me = meshes[m];
        if ((uint64_t)me.index_offset + me.index_count > n_indices || (uint64_t)me.vertex_offset + me.vertex_count > n_verts ||
            me.index_count % 3 != 0)
        {
            c->dev.err = "skh_set_geometry: mesh " + std::to_string(m) + " is out of range";
            return SKH_INVALID_ARGUMENT;
        }
        // indices are mesh-local (closest_hit.cu:365-376 adds mVbOffset): every one must address a vertex of its own mesh
        const uint32_t* ib = indices + me.index_offset;
        uint32_t worst = 0;
        for (uint32_t k = 0; k < me.index_count; ++k)
            worst = std::max(worst, ib[k]);
        if (me.index_count && worst >= me.vertex_count)
        {
            c->dev.err = "skh_set_geometry: mesh " + std::to_string(m) + " has index " + std::to_string(worst) + " >= its vertex_count " +
                     std::to_string(me.vertex_count);
            return SKH_INVALID_ARGUMENT;
        }
    }
    c->scene.meshes.assign(meshes, meshes + n_meshes);
    c->scene.nVerts = n_verts;
    c->scene.nIndices = n_indices;
    touched(c, skh_stale::IN_GEOMETRY);
    // signature of the TOPOLOGY (mesh table + index buffer): skh_refit_accel keeps the hierarchy only while it is the built one
    c->scene.geomSig = fnv1a_words(fnv1a_words(kFnv1aSeed, meshes, sizeof(skh_mesh) / 4 * (size_t)n_meshes), indices, n_indices) ^ ((uint64_t)n_verts << 32);
    skh_status s;
    if ((s = dev_upload(c, c->scene.dVerts, verts, sizeof(skh_vertex) * (size_t)n_verts)) != SKH_OK)
        return s;
    if ((s = dev_upload(c, c->scene.dIndices, indices, sizeof(uint32_t) * (size_t)n_indices)) != SKH_OK)
        return s;
    return dev_upload(c, c->scene.dMeshes, meshes, sizeof(skh_mesh) * (size_t)n_meshes);
}

skh_status skh_set_curves(skh_context* c, const float* points_xyz, uint32_t n_points, const float* radii, uint32_t n_radii,
                          const uint32_t* vertex_counts, uint32_t n_vertex_counts, const skh_curve* curves, uint32_t n_curves)
{
    if (!c || (n_points && !points_xyz) || (n_radii && !radii) || (n_vertex_counts && !vertex_counts) || (n_curves && !curves))
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    if (n_radii != n_points)
    {
        c->dev.err = "skh_set_curves: one radius per control point is required";
        return SKH_INVALID_ARGUMENT;
    }
    (void)hipSetDevice(c->dev.device);
    for (uint32_t k = 0; k < n_curves; ++k)
    {
        // ranges of oka::Curve (scene.h:29-42) against the arrays they address; the strands of a set must fit its point range
        const skh_curve& cu = curves[k];
        bool ok = (uint64_t)cu.vertex_counts_start + cu.vertex_counts_count <= n_vertex_counts &&
                  (uint64_t)cu.points_start + cu.points_count <= n_points && (uint64_t)cu.widths_start + cu.widths_count <= n_radii;
        uint64_t used = 0;
        for (uint32_t j = 0; ok && j < cu.vertex_counts_count; ++j)
            used += vertex_counts[cu.vertex_counts_start + j];
        if (!ok || used > cu.points_count)
        {
            c->dev.err = "skh_set_curves: curve set " + std::to_string(k) + " addresses data outside the arrays passed in";
            return SKH_INVALID_ARGUMENT;
        }
    }
    c->scene.curves.assign(curves, curves + n_curves);
    c->scene.curveVertexCounts.assign(vertex_counts, vertex_counts + n_vertex_counts);
    c->scene.nPoints = n_points;
    touched(c, skh_stale::IN_CURVES);
    // signature of the curve sets' TOPOLOGY (set table + vertex counts + array sizes): control points and radii may change under skh_refit_accel
    c->scene.curveSig = fnv1a_words(fnv1a_words(kFnv1aSeed, curves, sizeof(skh_curve) / 4 * (size_t)n_curves), vertex_counts, n_vertex_counts) ^ ((uint64_t)n_points << 32);
    skh_status s;
    if ((s = dev_upload(c, c->scene.dPoints, points_xyz, sizeof(float) * 3 * (size_t)n_points)) != SKH_OK)
        return s;
    return dev_upload(c, c->scene.dRadii, radii, sizeof(float) * (size_t)n_radii);
}

skh_status skh_set_instances(skh_context* c, const skh_instance* instances, uint32_t n)
{
    if (!c || (n && !instances))
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    // (skh_refit_accel compares the table with the build's: the same table again -- a caller that re-sends the whole scene with edited vertices -- keeps a refit
    // possible; skh_update_accel takes edited transforms in place)
    c->scene.instances.assign(instances, instances + n);
    c->scene.nInstances = n;
    touched(c, skh_stale::IN_INSTANCES);
    return dev_upload(c, c->scene.dInstances, instances, sizeof(skh_instance) * (size_t)n);
}

skh_status skh_set_lights(skh_context* c, const skh_light* lights, uint32_t n)
{
    if (!c || (n && !lights))
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    c->scene.nLights = n;
    c->scene.lightTypes.resize(n);
    for (uint32_t k = 0; k < n; ++k)
        c->scene.lightTypes[k] = lights[k].type;
    touched(c, skh_stale::IN_LIGHTS);
    return dev_upload(c, c->scene.dLights, lights, sizeof(skh_light) * (size_t)n);
}

static bool env_transform_ok(const float scale[3], const float w2e[9])
{
    for (int k = 0; k < 3; ++k)
        if (!(scale[k] >= 0.0f) || std::isinf(scale[k]))
            return false;
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(w2e[k]))
            return false;
    return true;
}

static EnvP make_env(const skh_context* c)
{
    EnvP e;
    memset(&e, 0, sizeof(e));
    if (c->env.w == 0)
        return e;
    e.texels = c->env.dTexels.as<float4>();
    e.rowCdf = c->env.dRowCdf.as<float>();
    e.colCdf = c->env.dColCdf.as<float>();
    e.width = c->env.w, e.height = c->env.h;
    e.pdfScale = (float)((double)c->env.w * (double)c->env.h / (2.0 * 3.14159265358979323846 * 3.14159265358979323846));
    e.nee = c->opt.envNee;
    memcpy(e.scale, c->env.scale, sizeof(e.scale));
    memcpy(e.w2e, c->env.w2e, sizeof(e.w2e));
    return e;
}

skh_status skh_set_environment(skh_context* c, const skh_environment* env)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    if (!env)
    {
        c->dev.err = "skh_set_environment: null description (rgb = NULL inside it removes the environment)";
        return SKH_INVALID_ARGUMENT;
    }
    (void)hipSetDevice(c->dev.device);
    if (!env->rgb)
    {
        // remove: a no-op on a context that has none (nothing traced ahead is thrown away for it)
        if (c->env.w == 0)
            return SKH_OK;
        spec_drop(c);
        SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
        dev_free(c->env.dTexels), dev_free(c->env.dColCdf), dev_free(c->env.dRowCdf);
        c->env.w = c->env.h = 0;
        c->env.sumW = c->env.msBuild = 0.0;
        return SKH_OK;
    }
    if (env->width < 2 || env->width > SKH_ENV_MAX_WIDTH || env->height < 2 || env->height > SKH_ENV_MAX_HEIGHT)
    {
        c->dev.err = "skh_set_environment: the map must be 2..8192 texels wide and 2..4096 high";
        return SKH_INVALID_ARGUMENT;
    }
    if (!env_transform_ok(env->scale, env->world_to_env))
    {
        c->dev.err = "skh_set_environment: scale must be finite and >= 0, world_to_env finite";
        return SKH_INVALID_ARGUMENT;
    }
    spec_drop(c);
    const uint32_t W = env->width, H = env->height;
    const size_t n = (size_t)W * H;
    // built beside the tables in use: a map that is refused leaves the previous environment as it was
    DevBuf dRgb, dTex, dCol, dRow, dTmp; // dTmp: H row sums (double), sum w (double), the bad-value flag
    SKH_CHECK(dev_upload(c, dRgb, env->rgb, n * 3 * sizeof(float)));
    SKH_CHECK(dev_alloc(c, dTex, n * sizeof(float4)));
    SKH_CHECK(dev_alloc(c, dCol, n * sizeof(float)));
    SKH_CHECK(dev_alloc(c, dRow, H * sizeof(float)));
    SKH_CHECK(dev_alloc(c, dTmp, (H + 2) * sizeof(double)));
    double* rowSum = dTmp.as<double>();
    double* sumW = rowSum + H;
    uint32_t* bad = reinterpret_cast<uint32_t*>(rowSum + H + 1);
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(double), c->dev.stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->dev.stream);
    const auto t0 = std::chrono::steady_clock::now();
    if (e == hipSuccess)
    {
        k_env_rows<<<H, SKH_ENV_BLOCK, 0, c->dev.stream>>>(dRgb.as<float>(), W, H, dTex.as<float4>(), dCol.as<float>(), rowSum, bad);
        k_env_marginal<<<1, SKH_ENV_BLOCK, 0, c->dev.stream>>>(rowSum, H, dRow.as<float>(), sumW);
        const uint32_t blocks = (uint32_t)std::min<size_t>((n + SKH_ENV_BLOCK - 1) / SKH_ENV_BLOCK, (size_t)c->dev.numCUs * 16u);
        k_env_normalise<<<blocks, SKH_ENV_BLOCK, 0, c->dev.stream>>>(dTex.as<float4>(), n, sumW);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->dev.stream);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    double total = 0.0;
    uint32_t badHost = 0;
    if (e == hipSuccess)
        e = hipMemcpy(&total, sumW, sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(&badHost, bad, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
    {
        c->dev.err = std::string("skh_set_environment: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? SKH_OUT_OF_MEMORY : SKH_FAIL;
    }
    if (badHost)
    {
        c->dev.err = "skh_set_environment: the map holds a negative or non-finite value";
        return SKH_INVALID_ARGUMENT;
    }
    c->env.dTexels = std::move(dTex), c->env.dColCdf = std::move(dCol), c->env.dRowCdf = std::move(dRow); // (the previous tables are freed here)
    c->env.w = W, c->env.h = H;
    memcpy(c->env.scale, env->scale, sizeof(c->env.scale));
    memcpy(c->env.w2e, env->world_to_env, sizeof(c->env.w2e));
    c->env.sumW = total;
    c->env.msBuild = ms;
    return SKH_OK;
}

skh_status skh_set_environment_transform(skh_context* c, const float scale[3], const float world_to_env[9])
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    if (!scale || !world_to_env || c->env.w == 0 || !env_transform_ok(scale, world_to_env))
    {
        c->dev.err = c->env.w == 0 ? "skh_set_environment_transform: the context has no environment" :
                                "skh_set_environment_transform: scale must be finite and >= 0, world_to_env finite";
        return SKH_INVALID_ARGUMENT;
    }
    spec_drop(c); // sub-frames traced ahead hold radiance of the old sky
    memcpy(c->env.scale, scale, sizeof(c->env.scale));
    memcpy(c->env.w2e, world_to_env, sizeof(c->env.w2e));
    return SKH_OK;
}

skh_status skh_get_environment_info(skh_context* c, skh_environment_info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->width = c->env.w, out->height = c->env.h;
    out->sum_w = c->env.sumW;
    out->ms_build = c->env.msBuild;
    out->bytes = c->env.w ? (uint64_t)c->env.w * c->env.h * (sizeof(float4) + sizeof(float)) + (uint64_t)c->env.h * sizeof(float) : 0u;
    return SKH_OK;
}

skh_status skh_set_textures(skh_context* c, const skh_texture* textures, uint32_t n)
{
    if (!c || (n && !textures))
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    std::vector<uint4> desc(n);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n; ++k)
    {
        if (!textures[k].rgba8 || textures[k].width == 0 || textures[k].height == 0)
        {
            c->dev.err = "skh_set_textures: texture " + std::to_string(k) + " is empty";
            return SKH_INVALID_ARGUMENT;
        }
        desc[k] = make_uint4((uint32_t)total, textures[k].width, textures[k].height, 0u);
        total += (uint64_t)textures[k].width * textures[k].height;
        if (total >= (1ull << 32))
        {
            c->dev.err = "skh_set_textures: more than 2^32 texels";
            return SKH_INVALID_ARGUMENT;
        }
    }
    std::vector<uint32_t> texels((size_t)total);
    for (uint32_t k = 0; k < n; ++k)
        memcpy(texels.data() + desc[k].x, textures[k].rgba8, (size_t)textures[k].width * textures[k].height * 4);
    skh_status s = dev_upload(c, c->scene.dTexels, texels.data(), sizeof(uint32_t) * texels.size());
    if (s == SKH_OK)
        s = dev_upload(c, c->scene.dTexDesc, desc.data(), sizeof(uint4) * desc.size());
    c->scene.nTextures = s == SKH_OK ? n : 0;
    touched(c, skh_stale::IN_TEXTURES);
    return s;
}
skh_status skh_set_materials(skh_context* c, const skh_material* materials, uint32_t n)
{
    if (!c || (n && !materials))
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    c->scene.nMaterials = n;
    touched(c, skh_stale::IN_MATERIALS);
    c->scene.hasHairMaterial = false;
    for (uint32_t k = 0; k < n; ++k)
        c->scene.hasHairMaterial = c->scene.hasHairMaterial || materials[k].type == SKH_MAT_HAIR;
    skh_status s = dev_upload(c, c->scene.dMaterials, materials, sizeof(skh_material) * (size_t)n);
    if (s != SKH_OK)
        return s;
    // the material-only terms of the hair BSDF, computed once per material ON THE DEVICE by the code the per-call path ran (skh_device.h hair_const)
    if ((s = dev_alloc(c, c->scene.dHairConst, sizeof(HairConst) * (size_t)std::max(1u, n))) != SKH_OK)
        return s;
    if (n)
        k_hair_consts<<<(n + 63) / 64, 64, 0, c->dev.stream>>>(c->scene.dMaterials.as<Material>(), n, c->scene.dHairConst.as<HairConst>());
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}

static skh_status build_shading_tables(skh_context* c)
{
    const uint32_t nMeshes = (uint32_t)c->scene.meshes.size();
    std::vector<uint32_t> base(nMeshes + 1u, 0u);
    uint64_t total = 0; // (summed wide and tested before narrowing: a 32-bit sum that wraps would pass the test below with aliased bases)
    for (uint32_t m = 0; m < nMeshes; ++m)
    {
        total += c->scene.meshes[m].index_count / 3u;
        base[m + 1] = (uint32_t)std::min<uint64_t>(total, 0xffffffffull);
    }
    const uint32_t nTris = base[nMeshes];
    c->accel.nShadeRecords = nTris;
    if (total >= SKH_PRIM_DIRECT)
    {
        c->dev.err = "skh_build_accel: more than 2^31 - 1 triangles (the primitive word of a hit keeps its top bit for SKH_PRIM_DIRECT)";
        return SKH_INVALID_ARGUMENT;
    }
    SKH_CHECK(dev_alloc(c, c->accel.dShadeTris, std::max<size_t>(96, (size_t)nTris * 96)));
    if (nTris)
    {
        DevBuf dBase;
        SKH_CHECK(dev_upload(c, dBase, base.data(), sizeof(uint32_t) * base.size()));
        k_gather_shade_tris<<<(nTris + 255u) / 256u, 256, 0, c->dev.stream>>>(c->scene.dVerts.as<uint8_t>(), c->scene.dIndices.as<uint32_t>(), c->scene.dMeshes.as<uint4>(),
                                                                         dBase.as<uint32_t>(), nMeshes, nTris, c->accel.dShadeTris.as<float4>());
        SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    }
    std::vector<skh_instance> inst = c->scene.instances;
    for (skh_instance& i : inst)
        if (i.type == SKH_INSTANCE_MESH)
            i.light_id = i.geom_id < nMeshes ? base[i.geom_id] : 0u;
    if (inst.empty())
        inst.resize(1);
    return dev_upload(c, c->accel.dShadeInst, inst.data(), sizeof(skh_instance) * inst.size());
}

#include "skh_accel.inc"


static size_t frame_count_words(const skh_context* c);

// k_raygen's tables for the context's tile list with the tiles of `frozenAt` (per tile, != 0: frozen; NULL: none) left out: valid slots per 512-slot block as an
// exclusive prefix sum, and their total
static void raygen_tables(const skh_context* c, const uint32_t* frozenAt, std::vector<uint32_t>& base, uint32_t& total)
{
    const uint32_t blocks = (c->frame.numSlots + 511u) / 512u, chunks = (uint32_t)c->frame.chunkValid.size(), shift2 = 2 * c->frame.tileShift;
    base.assign(std::max(1u, blocks), 0u);
    total = 0;
    for (uint32_t b = 0; b < blocks; ++b)
    {
        base[b] = total;
        for (uint32_t j = b * 8u; j < std::min(chunks, (b + 1) * 8u); ++j)
            if (!frozenAt || frozenAt[(j * 64u) >> shift2] == 0u)
                total += c->frame.chunkValid[j];
    }
}

// What k_raygen is given beside the frame: the two position tables, and how its grid walks the blocks.
struct RaygenOrder
{
    const uint32_t *qBase = nullptr, *subStride = nullptr; // (subStride NULL: the slot order)
    uint32_t launchCell = 1, perWave = 0;
};

// The cell size of queue_order 1 in raygen blocks (-1: a 64-slot chunk).  Automatic: the chunk -- the smallest cell was the fastest on the kitchen (docs/LOG.md
// "Queue order": 1/8, 1, 2, 4, 8, 16 blocks: -1.6, -1.0, -1.4, -0.7, -1.2, -0.3 % of the frame), and a cell of 64 pixels x 64 samples already fills four trace workgroups.
static int32_t cell_blocks(const skh_context* c)
{
    return c->opt.cellBlocks ? c->opt.cellBlocks : -1;
}

// k_raygen's order for a pass of `batch` sub-frames.  The slot order's tables are alloc_frame's (an adaptive pass's: adapt_after_pass's); the cell order's depend on the
// pass size and are built here the first time a pass of that size needs them: from the same per-chunk valid counts, with the same frozen tiles left out, so both
// orders fill exactly the positions [0, valid * batch).  A one-sub-frame pass has nothing to interleave: both options give it the slot order.
static skh_status raygen_order(skh_context* c, bool adaptive, uint32_t batch, RaygenOrder& out)
{
    skh_context::Frame& f = c->frame;
    out = RaygenOrder{};
    out.qBase = adaptive ? c->adapt.dRaygenBaseRender.as<uint32_t>() : f.dRaygenBase.as<uint32_t>();
    out.launchCell = std::max(1u, f.raygenBlocksPerSub);
    if (c->opt.queueOrder == 0u || batch <= 1u)
        return SKH_OK;
    const int32_t cb = cell_blocks(c);
    const uint32_t gen = adaptive ? c->adapt.orderGen : 0u;
    out.perWave = cb < 0 ? 1u : 0u;
    out.launchCell = cb < 0 ? 1u : std::min((uint32_t)cb, std::max(1u, f.raygenBlocksPerSub));
    skh_context::Frame::CellTables* e = nullptr;
    for (skh_context::Frame::CellTables& t : f.cellTables)
        if (t.batch == batch && t.cellBlocks == cb && t.adaptive == adaptive && t.gen == gen)
            e = &t;
    if (!e)
    {
        // the units: blocks, or their 64-slot chunks (padded to whole blocks); valid slots and first pixel of each, from the HOME list (a frozen tile counts nothing)
        const uint32_t perUnit = cb < 0 ? 1u : 8u, chunks = (uint32_t)f.chunkValid.size(), shift2 = 2 * f.tileShift, mask = (1u << shift2) - 1u;
        const uint32_t nUnits = f.raygenBlocksPerSub * (cb < 0 ? 8u : 1u);
        const uint32_t* frozenAt = adaptive ? c->adapt.frozenAt.data() : nullptr;
        std::vector<uint32_t> valid(nUnits, 0u), origin(2 * (size_t)nUnits, 0u);
        for (uint32_t u = 0; u < nUnits; ++u)
        {
            const uint32_t j0 = u * perUnit;
            if (j0 >= chunks)
                continue;
            const uint32_t tile = (j0 * 64u) >> shift2, m = (j0 * 64u) & mask;
            origin[2 * (size_t)u] = f.tileXY[2 * tile] + skh_order::even_bits(m), origin[2 * (size_t)u + 1] = f.tileXY[2 * tile + 1] + skh_order::even_bits(m >> 1);
            for (uint32_t j = j0; j < std::min(chunks, j0 + perUnit); ++j)
                if (!frozenAt || frozenAt[(j * 64u) >> shift2] == 0u)
                    valid[u] += f.chunkValid[j];
        }
        skh_order::Tables t;
        skh_order::cell_order(valid.data(), origin.data(), nUnits, batch, cb < 0 ? 1u : (uint32_t)cb, SKH_SHARDS, t);
        if (t.validPerSub != (adaptive ? c->adapt.raygenValid : f.raygenValidPerSub))
        {
            c->dev.err = "raygen_order: the cell order counts other slots than the slot order";
            return SKH_FAIL;
        }
        // a few pass sizes at most are alive at a time (the full batch, the tail of a call, the look-ahead's 2 / 4 / 8): beyond eight keys the oldest entry goes
        if (f.cellTables.size() < 8u)
            f.cellTables.emplace_back(), e = &f.cellTables.back();
        else
            e = &f.cellTables[f.cellTablesNext++ % 8u];
        e->batch = 0; // (not a key until both tables are up: dev_upload orders the copy behind the launches that read the old ones, and waits for it)
        SKH_CHECK(dev_upload(c, e->dQBase, t.qBase.data(), sizeof(uint32_t) * t.qBase.size()));
        SKH_CHECK(dev_upload(c, e->dSubStride, t.subStride.data(), sizeof(uint32_t) * t.subStride.size()));
        e->batch = batch, e->cellBlocks = cb, e->adaptive = adaptive, e->gen = gen;
    }
    out.qBase = e->dQBase.as<uint32_t>(), out.subStride = e->dSubStride.as<uint32_t>();
    return SKH_OK;
}

static skh_status alloc_frame(skh_context* c)
{
    const uint32_t T = c->frame.tileSize;
    c->frame.cellTables.clear(); // (of the frame that was)
    if (!c->frame.customTiles)
    {
        c->frame.tileXY.clear();
        for (uint32_t y = 0; y < c->frame.height; y += T)
            for (uint32_t x = 0; x < c->frame.width; x += T)
            {
                c->frame.tileXY.push_back(x);
                c->frame.tileXY.push_back(y);
            }
    }
    c->frame.numTiles = (uint32_t)(c->frame.tileXY.size() / 2);
    c->frame.numSlots = c->frame.numTiles * T * T;
    // sub-frame batching: aim at ~64 M paths per wavefront pass.  The persistent trace kernels have a long tail (a few
    // rays walk 10x the average number of nodes); at 2 M rays per launch the tail is half of the kernel time, at 64 M it
    // is amortised (measured at 1080p, Mray/s: 1 sub-frame per pass 1104, 16: 1942, 64: 2055 before the kernel work; with
    // the final kernels 8: 3455, 16: 3579, 32: 3678).  ~270 B per path: 18 GB of 288 GB at the default.
    c->frame.batchCapacity = c->opt.subframeBatch ? c->opt.subframeBatch : std::min(64u, std::max(1u, (1u << 27) / std::max(1u, c->frame.numSlots)));
    const size_t N1 = std::max(1u, c->frame.numSlots);
    const size_t N = N1 * c->frame.batchCapacity;
    // queues are sharded SKH_SHARDS ways: a shard's region holds an eighth of the paths (rounded up to whole waves); k_raygen deals the
    // first queue out in equal runs, and a k_shade workgroup emits into the shard it read from, so no shard outgrows its region
    c->frame.queueRegion = (uint32_t)((((N + SKH_SHARDS - 1) / SKH_SHARDS) + 63) & ~(size_t)63);
    const size_t NQ = (size_t)SKH_SHARDS * c->frame.queueRegion;
    SKH_CHECK(dev_upload(c, c->frame.dTileXY, c->frame.tileXY.data(), sizeof(uint32_t) * c->frame.tileXY.size()));
    {
        // valid (inside the image) slots per 64-slot chunk -- the 8 x 8 pixel block at the chunk's first pixel
        auto compact = [](uint32_t x) {
            x &= 0x55555555u;
            x = (x ^ (x >> 1)) & 0x33333333u;
            x = (x ^ (x >> 2)) & 0x0f0f0f0fu;
            x = (x ^ (x >> 4)) & 0x00ff00ffu;
            x = (x ^ (x >> 8)) & 0x0000ffffu;
            return x;
        };
        const uint32_t shift2 = 2 * c->frame.tileShift, mask = (1u << shift2) - 1u;
        c->frame.chunkValid.assign(c->frame.numSlots / 64u, 0u);
        for (uint32_t j = 0; j < c->frame.numSlots / 64u; ++j)
        {
            const uint32_t tile = (j * 64u) >> shift2, m = (j * 64u) & mask;
            const uint32_t x0 = c->frame.tileXY[2 * tile] + compact(m), y0 = c->frame.tileXY[2 * tile + 1] + compact(m >> 1);
            uint32_t n = 0;
            for (uint32_t k = 0; k < 64u; ++k)
                n += (x0 + compact(k) < c->frame.width && y0 + compact(k >> 1) < c->frame.height) ? 1u : 0u;
            c->frame.chunkValid[j] = n;
        }
        std::vector<uint32_t> base;
        raygen_tables(c, nullptr, base, c->frame.raygenValidPerSub);
        c->frame.raygenBlocksPerSub = (uint32_t)((c->frame.numSlots + 511u) / 512u);
        SKH_CHECK(dev_upload(c, c->frame.dRaygenBase, base.data(), sizeof(uint32_t) * base.size()));
    }
    c->adapt.ready = false; // (the feature's buffers follow the frame's: adapt_prepare)
    SKH_CHECK(dev_alloc(c, c->frame.dAccum, sizeof(float4) * N1));
    SKH_CHECK(dev_alloc(c, c->frame.dDiffuse, sizeof(float4) * N1));
    SKH_CHECK(dev_alloc(c, c->frame.dSpecular, sizeof(float4) * N1));
    SKH_CHECK(dev_alloc(c, c->frame.dDiffCnt, sizeof(uint16_t) * N1));
    SKH_CHECK(dev_alloc(c, c->frame.dSpecCnt, sizeof(uint16_t) * N1));
    SKH_CHECK(dev_alloc(c, c->frame.dSums, sizeof(float) * 11 * N1));
    SKH_CHECK(dev_alloc(c, c->frame.dPath, sizeof(float) * SKH_PATH_FLOATS * N));
    SKH_CHECK(dev_alloc(c, c->frame.dRayQ[0], sizeof(float) * 9 * NQ));
    SKH_CHECK(dev_alloc(c, c->frame.dRayQ[1], sizeof(float) * 9 * NQ));
    SKH_CHECK(dev_alloc(c, c->frame.dHits, sizeof(float) * 8 * NQ));
    SKH_CHECK(dev_alloc(c, c->frame.dShadowQ, sizeof(float) * 9 * NQ));
    SKH_CHECK(dev_alloc(c, c->frame.dContrib, sizeof(float4) * NQ));
    c->frame.queueConstFilled = false;
    SKH_CHECK(dev_alloc(c, c->frame.dCounts, sizeof(uint32_t) * frame_count_words(c)));
    c->frame.traceBlocks = (uint32_t)c->dev.numCUs * c->opt.wavesPerCU;
    SKH_CHECK(dev_alloc(c, c->frame.dOvf, sizeof(int) * (size_t)(SKH_STACK_OVF + SKH_TAIL_EXTRA) * (uint32_t)c->dev.numCUs * std::max(std::max(c->opt.wavesPerCU, c->opt.wavesPerCUWorld), std::max(c->opt.wavesPerCUShadow, c->opt.wavesPerCUShadowWorld)) * SKH_TRACE_BLOCK));
    SKH_CHECK(dev_alloc(c, c->frame.dOvf2, sizeof(int) * (size_t)(SKH_STACK_OVF + SKH_TAIL_EXTRA) * (uint32_t)c->dev.numCUs * std::max(std::max(c->opt.wavesPerCU, c->opt.wavesPerCUWorld), std::max(c->opt.wavesPerCUShadow, c->opt.wavesPerCUShadowWorld)) * SKH_TRACE_BLOCK));
    SKH_TRY(c, hipMemsetAsync(c->frame.dAccum.p, 0, sizeof(float4) * N1, c->dev.stream));
    SKH_TRY(c, hipMemsetAsync(c->frame.dDiffuse.p, 0, sizeof(float4) * N1, c->dev.stream));
    SKH_TRY(c, hipMemsetAsync(c->frame.dSpecular.p, 0, sizeof(float4) * N1, c->dev.stream));
    SKH_TRY(c, hipMemsetAsync(c->frame.dDiffCnt.p, 0, sizeof(uint16_t) * N1, c->dev.stream));
    SKH_TRY(c, hipMemsetAsync(c->frame.dSpecCnt.p, 0, sizeof(uint16_t) * N1, c->dev.stream));
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}

skh_status skh_resize(skh_context* c, uint32_t width, uint32_t height)
{
    if (!c || width == 0 || height == 0)
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    c->frame.width = width;
    c->frame.height = height;
    return alloc_frame(c);
}

skh_status skh_set_tiles(skh_context* c, uint32_t tile_size, const uint32_t* tile_xy, uint32_t n_tiles)
{
    if (!c || tile_size < 8 || tile_size > 256 || (tile_size & (tile_size - 1)))
        return SKH_INVALID_ARGUMENT;
    spec_drop(c);
    (void)hipSetDevice(c->dev.device);
    c->frame.tileSize = tile_size;
    c->frame.tileShift = 0;
    while ((1u << c->frame.tileShift) < tile_size)
        ++c->frame.tileShift;
    c->frame.customTiles = tile_xy != nullptr;
    if (tile_xy)
        c->frame.tileXY.assign(tile_xy, tile_xy + 2 * (size_t)n_tiles);
    if (c->frame.width && c->frame.height)
        return alloc_frame(c);
    return SKH_OK;
}

// ---- timing helpers ----
static hipEvent_t next_event(skh_context* c)
{
    if (c->timing.eventsUsed == c->timing.eventPool.size())
    {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        c->timing.eventPool.push_back(e);
    }
    return c->timing.eventPool[c->timing.eventsUsed++];
}
struct SpanGuard
{
    skh_context* c;
    int cls;
    hipEvent_t a = nullptr;
    hipStream_t st;
    SpanGuard(skh_context* c_, int cls_, hipStream_t st_ = nullptr) : c(c_), cls(cls_), st(st_ ? st_ : c_->dev.stream)
    {
        c->timing.launches[cls]++;
        if (c->opt.timing)
        {
            a = next_event(c);
            (void)hipEventRecord(a, st);
        }
    }
    ~SpanGuard()
    {
        if (c->opt.timing)
        {
            hipEvent_t b = next_event(c);
            (void)hipEventRecord(b, st);
            c->timing.spans.push_back(TimedSpan{ cls, a, b });
        }
    }
};
static void harvest_spans(skh_context* c)
{
    for (const TimedSpan& s : c->timing.spans)
    {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess)
        {
            c->timing.msClass[s.cls] += ms;
            if (getenv("SKH_DEBUG_SPANS"))
                fprintf(stderr, "[span] class %d %.3f ms\n", s.cls, ms);
        }
    }
    c->timing.spans.clear();
    c->timing.eventsUsed = 0;
}

static DevScene make_dev_scene(const skh_context* c)
{
    DevScene sc;
    sc.tlasNodes = c->accel.dTlasNodes.as<Node4>();
    sc.tlasInst = c->accel.dTlasInst.as<uint32_t>();
    sc.tlasRoot = c->accel.tlasRoot;
    sc.numWorldCurves = c->accel.numWorldCurves;
    sc.worldCurveIdentLast = c->accel.worldCurveIdentLast;
    sc.worldCurveMerged = c->accel.worldCurveMerged;
    for (uint32_t k = 0; k < SKH_WORLD_CURVES; ++k)
        sc.worldCurveRoot[k] = k < c->accel.numWorldCurves ? c->accel.worldCurveRoot[k] : SKH_REF_INVALID, sc.worldCurveInst[k] = k < c->accel.numWorldCurves ? c->accel.worldCurveInst[k] : 0u;
    sc.numInstances = c->scene.nInstances;
    sc.inst = c->accel.dDevInst.as<DevInstance>();
    sc.tinst = c->accel.dTravInst.as<DevInstance>();
    sc.triNodes = c->accel.dTriNodes.as<Node4>();
    sc.tris = c->accel.dTris.as<float4>();
    sc.segNodes = c->accel.dSegNodes.as<Node4>();
    sc.segs = c->accel.dSegs.as<float4>();
    sc.curveSplit = c->accel.curveSplitBuilt;
    sc.worldRoot = c->accel.worldRoot;
    sc.lightRoot = c->accel.lightRoot;
    sc.instances = c->accel.dShadeInst.as<HostInstance>();
    sc.shadeTris = c->accel.dShadeTris.as<float4>();
    sc.verts = c->scene.dVerts.as<uint8_t>();
    sc.indices = c->scene.dIndices.as<uint32_t>();
    sc.meshes = c->scene.dMeshes.as<uint4>();
    sc.curveSegBase = c->accel.dCurveSegBase.as<uint32_t>();
    sc.segStartAll = c->accel.dSegStartAll.as<uint32_t>();
    sc.cpoints = c->scene.dPoints.as<float>();
    sc.cradii = c->scene.dRadii.as<float>();
    sc.lights = c->scene.dLights.as<Light>();
    sc.numLights = c->scene.nLights;
    sc.materials = c->scene.dMaterials.as<Material>();
    sc.hairConst = c->scene.dHairConst.as<HairConst>();
    sc.numMaterials = c->scene.nMaterials;
    sc.texels = c->scene.dTexels.as<uint32_t>();
    sc.texDesc = c->scene.dTexDesc.as<uint4>();
    sc.numTextures = c->scene.nTextures;
    sc.profile = c->timing.dStats.as<StatsDev>();
    sc.overflowFlag = c->dev.hOverflow; // (hipHostMallocMapped memory: the host pointer is valid on the device)
    return sc;
}

// What the probes (tests' doors to single device functions) share: the inputs up (an input without bytes is left out), the output allocated, `launch(dIn, dOut)`
// on c->dev.stream, the launch checked, the stream waited for, the output back.
struct ProbeIn
{
    const void* src;
    size_t bytes;
};
template <size_t N, typename Launch>
static skh_status probe_roundtrip(skh_context* c, const ProbeIn (&in)[N], void* out, size_t outBytes, Launch&& launch)
{
    DevBuf dIn[N], dOut;
    for (size_t k = 0; k < N; ++k)
        if (in[k].bytes)
            SKH_CHECK(dev_upload(c, dIn[k], in[k].src, in[k].bytes));
    SKH_CHECK(dev_alloc(c, dOut, outBytes));
    launch(dIn, dOut);
    SKH_TRY(c, hipGetLastError());
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    SKH_TRY(c, hipMemcpy(out, dOut.p, outBytes, hipMemcpyDeviceToHost));
    return SKH_OK;
}

// ---- material textures: skh_set_material_textures ----
// an entry binds a texture that exists: the k_shade builds with MTEX in them run (anything else -- no table, all ids 0 or beyond the list -- runs the others)
static bool mtex_active(const skh_context* c)
{
    for (const skh_material_textures& e : c->mtex.table)
        for (uint32_t id : { e.roughness_texture, e.metallic_texture, e.emission_texture })
            if (id != 0u && id <= c->scene.nTextures)
                return true;
    return false;
}

static MtexP make_mtex(const skh_context* c)
{
    MtexP m;
    m.table = nullptr, m.count = 0;
    if (mtex_active(c))
        m.table = c->mtex.dTable.as<uint4>(), m.count = (uint32_t)c->mtex.table.size();
    return m;
}

// What the per-material table setters share.  Removal (no entries) is a no-op on a context that has none: nothing traced ahead is thrown away for it.  `check` validates
// the entries, leaves the message of a refusal, and may point `src` / `bytes` at a packed form of the table; `changed`: the input this table is (skh_stale.h).
template <typename T, typename Check>
static skh_status set_material_table(skh_context* c, const char* fn, const T* entries, uint32_t n, std::vector<T>& kept, DevBuf& dev, skh_stale::Input changed, Check&& check)
{
    (void)hipSetDevice(c->dev.device);
    const void* src = entries;
    size_t bytes = sizeof(T) * (size_t)n;
    if (entries && n > c->scene.nMaterials)
    {
        c->dev.err = std::string(fn) + ": " + std::to_string(n) + " entries for " + std::to_string(c->scene.nMaterials) + " materials (call skh_set_materials first)";
        return SKH_INVALID_ARGUMENT;
    }
    if (!entries || n == 0)
    {
        if (kept.empty())
            return SKH_OK;
    }
    else
        SKH_CHECK(check(src, bytes));
    spec_drop(c);
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream)); // (the table is about to be replaced)
    DevBuf d;
    if (entries && n)
    {
        SKH_CHECK(dev_upload(c, d, src, bytes));
        kept.assign(entries, entries + n);
    }
    else
        kept.clear();
    dev = std::move(d);
    touched(c, changed);
    return SKH_OK;
}

skh_status skh_set_material_textures(skh_context* c, const skh_material_textures* entries, uint32_t n)
{
    static_assert(sizeof(skh_material_textures) == 48 && sizeof(skh_material_textures) == sizeof(MtexEntry), "skh_material_textures");
    if (!c)
        return SKH_INVALID_ARGUMENT;
    return set_material_table(c, "skh_set_material_textures", entries, n, c->mtex.table, c->mtex.dTable, skh_stale::IN_MATERIAL_TEXTURES, [&](const void*&, size_t&) {
        for (uint32_t k = 0; k < n; ++k)
        {
            const skh_material_textures& e = entries[k];
            if (e.roughness_channel > 3u || e.metallic_channel > 3u || e.emission_channel > 4u || !std::isfinite(e.roughness_scale) || !std::isfinite(e.roughness_bias) ||
                !std::isfinite(e.metallic_scale) || !std::isfinite(e.metallic_bias) || e.reserved[0] != 0u || e.reserved[1] != 0u)
            {
                c->dev.err = "skh_set_material_textures: entry " + std::to_string(k) + ": a channel out of range (0..3, emission 0..4), a scale or bias that is not finite, or a non-zero reserved word";
                return SKH_INVALID_ARGUMENT;
            }
        }
        return SKH_OK;
    });
}

skh_status skh_material_probe(skh_context* c, uint32_t n, const uint32_t* material, const float* uv, float* out)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    if (n && (!material || !uv || !out))
    {
        c->dev.err = "skh_material_probe: a missing input / output pointer";
        return SKH_INVALID_ARGUMENT;
    }
    if (c->scene.nMaterials == 0)
    {
        c->dev.err = "skh_material_probe: the context has no materials (call skh_set_materials first)";
        return SKH_INVALID_ARGUMENT;
    }
    if (n == 0)
        return SKH_OK;
    (void)hipSetDevice(c->dev.device);
    std::vector<float> le(4 * (size_t)c->scene.nMaterials, 0.0f); // (materials beyond the emission list do not emit)
    for (uint32_t m = 0; m < c->scene.nMaterials && 3 * (size_t)m + 2 < c->emit.emission.size(); ++m)
        memcpy(&le[4 * (size_t)m], &c->emit.emission[3 * (size_t)m], 3 * sizeof(float));
    const ProbeIn in[] = { { le.data(), le.size() * sizeof(float) }, { material, sizeof(uint32_t) * (size_t)n }, { uv, 2 * sizeof(float) * (size_t)n } };
    return probe_roundtrip(c, in, out, 8 * sizeof(float) * (size_t)n, [&](const DevBuf* d, const DevBuf& dOut) {
        k_material_probe<<<(n + 255) / 256, 256, 0, c->dev.stream>>>(make_mtex(c), c->scene.dMaterials.as<Material>(), c->scene.nMaterials, d[0].as<float4>(), c->scene.dTexels.as<uint32_t>(),
                                                                 c->scene.dTexDesc.as<uint4>(), c->scene.nTextures, d[1].as<uint32_t>(), d[2].as<float>(), n, dOut.as<float>());
    });
}

// ---- cutouts: skh_set_material_cutouts, the k_cutout stage between trace and shade (skh_kernels.h) ----
static_assert(sizeof(skh_material_cutout) == 32, "skh_material_cutout");
#define SKH_CUT_WORDS (SKH_COUNT_STRIDE * SKH_SHARDS + 8 * SKH_FETCH_STRIDE) // per continuation round: the queue's length words, the trace launch's fetch cursors

skh_status skh_set_material_cutouts(skh_context* c, const skh_material_cutout* entries, uint32_t n)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    return set_material_table(c, "skh_set_material_cutouts", entries, n, c->cut.cutouts, c->cut.dCutouts, skh_stale::IN_MATERIAL_CUTOUTS, [&](const void*&, size_t&) {
        for (uint32_t k = 0; k < n; ++k)
        {
            const skh_material_cutout& e = entries[k];
            if (e.opacity_channel > 3u || !std::isfinite(e.opacity_scale) || !std::isfinite(e.opacity_bias) || !(e.threshold >= 0.0f && e.threshold <= 1.0f) ||
                e.reserved[0] != 0u || e.reserved[1] != 0u || e.reserved[2] != 0u)
            {
                c->dev.err = "skh_set_material_cutouts: entry " + std::to_string(k) + ": a channel above 3, a scale or bias that is not finite, a threshold outside [0, 1] or a non-zero reserved word";
                return SKH_INVALID_ARGUMENT;
            }
        }
        return SKH_OK;
    });
}

// ---- fractional opacity: skh_set_material_blend, the BLEND build of k_cutout (skh_kernels.h) ----
static_assert(sizeof(skh_material_blend) == 32, "skh_material_blend");

skh_status skh_set_material_blend(skh_context* c, const skh_material_blend* entries, uint32_t n)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    std::vector<uint4> packed; // what the device reads: one uint4 per material (BlendP)
    return set_material_table(c, "skh_set_material_blend", entries, n, c->cut.blends, c->cut.dBlend, skh_stale::IN_MATERIAL_BLEND, [&](const void*& src, size_t& bytes) {
        packed.resize(n);
        for (uint32_t k = 0; k < n; ++k)
        {
            const skh_material_blend& e = entries[k];
            if (e.opacity_channel > 3u || !std::isfinite(e.opacity_scale) || !std::isfinite(e.opacity_bias) || e.active > 1u || e.reserved[0] != 0u || e.reserved[1] != 0u ||
                e.reserved[2] != 0u)
            {
                c->dev.err = "skh_set_material_blend: material " + std::to_string(k) + ": a channel above 3, a scale or bias that is not finite, active above 1 or a non-zero reserved word";
                return SKH_INVALID_ARGUMENT;
            }
            uint32_t sb, bb;
            memcpy(&sb, &e.opacity_scale, 4);
            memcpy(&bb, &e.opacity_bias, 4);
            packed[k] = make_uint4(e.opacity_texture, e.opacity_channel | (e.active << 31), sb, bb);
        }
        src = packed.data(), bytes = sizeof(uint4) * (size_t)n;
        return SKH_OK;
    });
}

// the material an instance shades with, as k_shade reads it
static inline uint32_t instance_material(const skh_context* c, const skh_instance& in)
{
    const uint32_t mid = in.material_id == 0xffffffffu ? 0u : in.material_id;
    return mid < c->scene.nMaterials ? mid : 0u;
}

// does material k emit (skh_set_emission)?
static inline bool material_emits(const skh_context* c, size_t k)
{
    return 3 * k + 2 < c->emit.emission.size() && (c->emit.emission[3 * k] > 0.0f || c->emit.emission[3 * k + 1] > 0.0f || c->emit.emission[3 * k + 2] > 0.0f);
}

// the active entries among the first n of a per-material table, and the mesh instances that use one
template <typename Active>
static void count_in_use(const skh_context* c, uint32_t n, Active&& active, uint32_t& entries, uint32_t& users)
{
    entries = users = 0;
    for (uint32_t k = 0; k < n; ++k)
        entries += active(k) ? 1u : 0u;
    if (entries)
        for (const skh_instance& in : c->scene.instances)
            users += (in.type == SKH_INSTANCE_MESH && instance_material(c, in) < n && active(instance_material(c, in))) ? 1u : 0u;
}

// Is a cutout in use (derived: an active entry on a material that a mesh instance uses)?  And the one combination that is refused: a material that emits and is cut.
static skh_status cut_ensure(skh_context* c)
{
    if (c->cut.stale)
    {
        const uint32_t nTab = (uint32_t)std::min<size_t>(c->cut.cutouts.size(), c->scene.nMaterials);
        count_in_use(c, nTab, [&](uint32_t k) { return c->cut.cutouts[k].threshold > 0.0f; }, c->cut.activeMaterials, c->cut.instances);
        // fractional opacity: the same derivation over the blend table
        const uint32_t nBl = (uint32_t)std::min<size_t>(c->cut.blends.size(), c->scene.nMaterials);
        count_in_use(c, nBl, [&](uint32_t k) { return c->cut.blends[k].active != 0u; }, c->cut.blendActiveMaterials, c->cut.blendInstances);
        c->cut.stale = false;
    }
    if (c->cut.blendActiveMaterials)
        for (uint32_t k = 0; k < c->cut.blends.size() && k < c->scene.nMaterials; ++k)
        {
            if (!c->cut.blends[k].active)
                continue;
            if (k < c->cut.cutouts.size() && c->cut.cutouts[k].threshold > 0.0f)
            {
                c->dev.err = "material " + std::to_string(k) + " has both an active cutout (skh_set_material_cutouts) and an active blend entry (skh_set_material_blend): one opacity rule per material";
                return SKH_INVALID_ARGUMENT;
            }
            if (material_emits(c, k))
            {
                c->dev.err = "material " + std::to_string(k) + " both emits (skh_set_emission) and has an active blend entry (skh_set_material_blend): blended emitters are not supported";
                return SKH_INVALID_ARGUMENT;
            }
        }
    if (c->cut.activeMaterials && !c->emit.emission.empty())
        for (uint32_t k = 0; k < c->cut.cutouts.size() && k < c->scene.nMaterials; ++k)
            if (c->cut.cutouts[k].threshold > 0.0f && material_emits(c, k))
            {
                c->dev.err = "material " + std::to_string(k) + " both emits (skh_set_emission) and has an active cutout (skh_set_material_cutouts): cut-away emitters are not supported";
                return SKH_INVALID_ARGUMENT;
            }
    return SKH_OK;
}

// does the stage between trace and shade run: is a cutout or a blend entry in use?
static inline bool cut_stage_on(const skh_context* c)
{
    return c->cut.instances != 0u || c->cut.blendInstances != 0u;
}

static CutoutP make_cutout(const skh_context* c)
{
    CutoutP p;
    p.table = c->cut.dCutouts.as<uint4>();
    p.count = (uint32_t)std::min<size_t>(c->cut.cutouts.size(), c->scene.nMaterials);
    return p;
}

// the part of BlendP a context fixes; the caller adds what the launch fixes (raw or depth and the frame's constants, the contribution records), the chain the round
static BlendP make_blend(const skh_context* c)
{
    BlendP p;
    memset(&p, 0, sizeof(p));
    if (c->cut.blendInstances)
    {
        p.table = c->cut.dBlend.as<uint4>();
        p.count = (uint32_t)std::min<size_t>(c->cut.blends.size(), c->scene.nMaterials);
    }
    return p;
}

static size_t frame_count_words(const skh_context* c)
{
    const size_t base = (size_t)SKH_COUNT_STRIDE * SKH_SHARDS * 2 * SKH_MAX_LAUNCH_ROUNDS + (size_t)16 * SKH_FETCH_STRIDE * SKH_MAX_LAUNCH_ROUNDS;
    // behind them, in a context with a cutout in use: per bounce and side (closest, shadow) cutout_rounds x {length words, fetch cursors}
    return base + (cut_stage_on(c) ? (size_t)SKH_MAX_LAUNCH_ROUNDS * 2 * c->opt.cutoutRounds * SKH_CUT_WORDS : 0u);
}

// the cutout stage's frame buffers: allocated when a cutout is in use (and only then), freed when none is any more
static skh_status cut_alloc_frame(skh_context* c)
{
    if (!cut_stage_on(c))
    {
        if (c->cut.dQ[0].p)
        {
            SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
            for (int k = 0; k < 2; ++k)
                dev_free(c->cut.dQ[k]), dev_free(c->cut.dShadowQ[k]), dev_free(c->cut.dShadowHits[k]);
            dev_free(c->cut.dHits);
        }
        return SKH_OK;
    }
    if (!c->frame.width)
        return SKH_OK;
    const size_t NQ = (size_t)SKH_SHARDS * c->frame.queueRegion;
    const size_t qBytes = sizeof(float) * 9 * NQ, hBytes = sizeof(float) * 8 * NQ, cBytes = sizeof(uint32_t) * frame_count_words(c);
    if (c->cut.dQ[0].bytes >= qBytes && c->cut.dQ[0].bytes <= 2 * qBytes + 4096 && c->frame.dCounts.bytes >= cBytes)
        return SKH_OK;
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    for (int k = 0; k < 2; ++k)
    {
        SKH_CHECK(dev_alloc(c, c->cut.dQ[k], qBytes));
        SKH_CHECK(dev_alloc(c, c->cut.dShadowQ[k], qBytes));
        SKH_CHECK(dev_alloc(c, c->cut.dShadowHits[k], hBytes));
    }
    SKH_CHECK(dev_alloc(c, c->cut.dHits, hBytes));
    if (c->frame.dCounts.bytes < cBytes)
        SKH_CHECK(dev_alloc(c, c->frame.dCounts, cBytes));
    return SKH_OK;
}

// bytes of the cutout stage's frame buffers
static uint64_t cut_stage_bytes(const skh_context* c)
{
    return c->cut.dQ[0].bytes + c->cut.dQ[1].bytes + c->cut.dHits.bytes + c->cut.dShadowQ[0].bytes + c->cut.dShadowQ[1].bytes + c->cut.dShadowHits[0].bytes + c->cut.dShadowHits[1].bytes;
}

// what skh_get_cutout_info and skh_get_blend_info share: the in-use counts brought up to date, the stage's counters read back
static skh_status cut_read_stats(skh_context* c, CutStatsDev& sd)
{
    (void)hipSetDevice(c->dev.device);
    SKH_CHECK(cut_ensure(c));
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    SKH_TRY(c, hipMemcpy(&sd, c->cut.dStats.p, sizeof(sd), hipMemcpyDeviceToHost));
    return SKH_OK;
}

skh_status skh_get_cutout_info(skh_context* c, skh_cutout_info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    CutStatsDev sd;
    SKH_CHECK(cut_read_stats(c, sd));
    out->active_materials = c->cut.activeMaterials, out->instances = c->cut.instances;
    out->continued_closest = sd.continued[0], out->continued_shadow = sd.continued[1];
    out->accepted_by_cap = sd.capped[0] + sd.capped[1];
    out->bytes = cut_stage_bytes(c);
    return SKH_OK;
}

skh_status skh_get_blend_info(skh_context* c, skh_blend_info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    CutStatsDev sd;
    SKH_CHECK(cut_read_stats(c, sd));
    out->active_materials = c->cut.blendActiveMaterials, out->instances = c->cut.blendInstances;
    out->passed_radiance = sd.blendPassed, out->crossed_shadow = sd.blendCrossed, out->accepted_by_cap = sd.blendCapped;
    out->bytes = cut_stage_bytes(c);
    return SKH_OK;
}

skh_status skh_blend_probe(skh_context* c, uint32_t n, const uint32_t* in, float* xi)
{
    if (!c || (n && (!in || !xi)))
        return SKH_INVALID_ARGUMENT;
    if (!n)
        return SKH_OK;
    (void)hipSetDevice(c->dev.device);
    const ProbeIn pin[] = { { in, sizeof(uint32_t) * 6 * (size_t)n } };
    return probe_roundtrip(c, pin, xi, sizeof(float) * (size_t)n,
                           [&](const DevBuf* d, const DevBuf& dOut) { k_blend_probe<<<(n + 255) / 256, 256, 0, c->dev.stream>>>(n, d[0].as<uint32_t>(), dOut.as<float>()); });
}

static skh_status ensure_ready(skh_context* c);

// ---- light shapes: skh_set_light_shapes, the LSHAPE builds of k_shade (skh_lshape.h, skh_device.h) ----
static_assert(sizeof(skh_light_shape) == 32, "skh_light_shape");
static_assert(SKH_LIGHT_SHAPE_SAMPLE_DISC == SKH_LSHAPE_SAMPLE_DISC && SKH_LIGHT_SHAPE_CONE == SKH_LSHAPE_CONE, "the flags of the ABI are the device's");

// the flags of an entry that apply to a light of this type
static uint32_t lshape_flags_for(uint32_t flags, int32_t type)
{
    return flags & ((type == 1 ? SKH_LIGHT_SHAPE_SAMPLE_DISC : 0u) | ((type == 0 || type == 1 || type == 2) ? SKH_LIGHT_SHAPE_CONE : 0u));
}

// Which entries are in use (derived: after skh_set_lights and skh_set_light_shapes)?  The device table -- one entry per light, flags masked to those in use, zeros
// for lights beyond the caller's table -- exists only when one is.
static skh_status lshape_ensure(skh_context* c)
{
    if (!c->lshape.stale)
        return SKH_OK;
    const uint32_t n = (uint32_t)std::min<size_t>(c->lshape.table.size(), c->scene.nLights);
    uint32_t discs = 0, cones = 0;
    std::vector<float> table(8 * (size_t)c->scene.nLights, 0.0f);
    for (uint32_t k = 0; k < n; ++k)
    {
        const skh_light_shape& e = c->lshape.table[k];
        const uint32_t f = lshape_flags_for(e.flags, c->scene.lightTypes[k]);
        discs += (f & SKH_LIGHT_SHAPE_SAMPLE_DISC) ? 1u : 0u, cones += (f & SKH_LIGHT_SHAPE_CONE) ? 1u : 0u;
        float* o = &table[8 * (size_t)k];
        memcpy(o, &f, 4);
        o[1] = e.cos_outer, o[2] = e.cos_inner, o[3] = e.focus, o[4] = e.axis[0], o[5] = e.axis[1], o[6] = e.axis[2];
    }
    if (c->lshape.dTable.p || discs || cones)
        SKH_TRY(c, hipStreamSynchronize(c->dev.stream)); // (the table is about to be replaced or freed)
    if (discs || cones)
    {
        DevBuf d;
        SKH_CHECK(dev_upload(c, d, table.data(), table.size() * sizeof(float)));
        c->lshape.dTable = std::move(d);
    }
    else
        dev_free(c->lshape.dTable);
    c->lshape.discs = discs, c->lshape.cones = cones;
    c->lshape.stale = false;
    return SKH_OK;
}

static LshapeP make_lshape(const skh_context* c)
{
    LshapeP p;
    p.table = (c->lshape.discs || c->lshape.cones) ? c->lshape.dTable.as<float4>() : nullptr;
    return p;
}

skh_status skh_set_light_shapes(skh_context* c, const skh_light_shape* entries, uint32_t n)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (!entries || n == 0)
    {
        // remove: a no-op on a context that has none (nothing traced ahead is thrown away for it)
        if (c->lshape.table.empty())
            return SKH_OK;
        spec_drop(c);
        c->lshape.table.clear();
        touched(c, skh_stale::IN_LIGHT_SHAPES);
        return SKH_OK;
    }
    if (n > c->scene.nLights)
    {
        c->dev.err = "skh_set_light_shapes: " + std::to_string(n) + " entries for " + std::to_string(c->scene.nLights) + " lights (call skh_set_lights first)";
        return SKH_INVALID_ARGUMENT;
    }
    for (uint32_t k = 0; k < n; ++k)
    {
        const skh_light_shape& e = entries[k];
        bool ok = e.flags <= 3u && e.reserved == 0u && std::isfinite(e.cos_outer) && std::isfinite(e.cos_inner) && e.cos_outer >= -1.0f && e.cos_outer <= 1.0f &&
                  e.cos_inner >= -1.0f && e.cos_inner <= 1.0f && e.cos_inner >= e.cos_outer && std::isfinite(e.focus) && e.focus >= 0.0f;
        if (ok && (e.flags & SKH_LIGHT_SHAPE_CONE))
        {
            const double len = std::sqrt((double)e.axis[0] * e.axis[0] + (double)e.axis[1] * e.axis[1] + (double)e.axis[2] * e.axis[2]);
            ok = std::isfinite(e.axis[0]) && std::isfinite(e.axis[1]) && std::isfinite(e.axis[2]) && std::fabs(len - 1.0) <= 1e-3;
        }
        if (!ok)
        {
            c->dev.err = "skh_set_light_shapes: light " + std::to_string(k) +
                     ": flags above 3, a cosine outside [-1, 1] or not finite, cos_inner < cos_outer, a focus that is negative or not finite, a cone axis that is not "
                     "finite or not of unit length, or a non-zero reserved word";
            return SKH_INVALID_ARGUMENT;
        }
    }
    spec_drop(c);
    c->lshape.table.assign(entries, entries + n);
    touched(c, skh_stale::IN_LIGHT_SHAPES);
    return SKH_OK;
}

skh_status skh_get_light_shape_info(skh_context* c, skh_light_shape_info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    (void)hipSetDevice(c->dev.device);
    SKH_CHECK(lshape_ensure(c));
    out->sampled_discs = c->lshape.discs, out->cones = c->lshape.cones;
    return SKH_OK;
}

skh_status skh_light_shape_probe(skh_context* c, uint32_t kind, const void* in, uint32_t n, void* out)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    if (kind > SKH_LSHAPE_PROBE_PDF || (n && (!in || !out)))
    {
        c->dev.err = "skh_light_shape_probe: unknown kind, or a missing input / output pointer";
        return SKH_INVALID_ARGUMENT;
    }
    (void)hipSetDevice(c->dev.device);
    SKH_CHECK(lshape_ensure(c));
    if (n == 0)
        return SKH_OK;
    const size_t inBytes = (kind == SKH_LSHAPE_PROBE_SAMPLE ? 6u : 7u) * sizeof(uint32_t), outBytes = (kind == SKH_LSHAPE_PROBE_SAMPLE ? 13u : 2u) * sizeof(float);
    const ProbeIn pin[] = { { in, inBytes * n } };
    return probe_roundtrip(c, pin, out, outBytes * n, [&](const DevBuf* d, const DevBuf& dOut) {
        k_lshape_probe<<<(n + 255) / 256, 256, 0, c->dev.stream>>>(c->scene.dLights.as<Light>(), c->scene.nLights, make_lshape(c), 0u, kind, d[0].as<uint32_t>(), n, dOut.as<float>());
    });
}

// ---- emissive meshes: skh_set_emission, the emitter table (skh_emit.h) ----
static void emit_clear(skh_context* c)
{
    dev_free(c->emit.dEntries), dev_free(c->emit.dCdf), dev_free(c->emit.dGuide), dev_free(c->emit.dLe), dev_free(c->emit.dInstOffset);
    c->emit.count = c->emit.instances = c->emit.guideBits = 0;
    c->emit.sumW = 0.0;
}

static float lum709(const float* rgb)
{
    return (float)(0.2126 * (double)rgb[0] + 0.7152 * (double)rgb[1] + 0.0722 * (double)rgb[2]);
}

// Builds the table when it is stale.  Needs the geometry, the instances and the material count, no acceleration structure.
static skh_status emit_ensure(skh_context* c)
{
    if (!c->emit.stale)
        return SKH_OK;
    if (c->emit.emission.empty())
    {
        // (nothing emits: no device work, no synchronisation -- a context that was never told pays one test per call)
        if (c->emit.count || c->emit.dLe.p)
        {
            SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
            emit_clear(c);
        }
        c->emit.msBuild = 0.0;
        c->emit.stale = false;
        return SKH_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream)); // (the tables are about to be replaced)
    const uint32_t nMat = std::max(1u, c->scene.nMaterials), nMeshes = (uint32_t)c->scene.meshes.size(), nInst = (uint32_t)c->scene.instances.size();
    std::vector<float> le(4 * (size_t)nMat, 0.0f); // {r, g, b, luminance}; materials beyond the emission list do not emit
    for (uint32_t m = 0; m < nMat && 3 * (size_t)m + 2 < c->emit.emission.size(); ++m)
    {
        memcpy(&le[4 * (size_t)m], &c->emit.emission[3 * (size_t)m], 3 * sizeof(float));
        le[4 * (size_t)m + 3] = lum709(&c->emit.emission[3 * (size_t)m]);
    }
    std::vector<uint32_t> emitInst, emitBase, instOffset(std::max(1u, nInst), 0xffffffffu);
    uint64_t total = 0;
    for (uint32_t i = 0; i < nInst; ++i)
    {
        const skh_instance& in = c->scene.instances[i];
        if (in.type != SKH_INSTANCE_MESH || in.geom_id >= nMeshes)
            continue;
        const uint32_t mid = instance_material(c, in);
        float w2o[12];
        const uint32_t tris = c->scene.meshes[in.geom_id].index_count / 3u;
        if (!(le[4 * (size_t)mid + 3] > 0.0f) || tris == 0 || !invert_affine(in.transform, w2o)) // (a singular instance is disabled: no ray reaches it)
            continue;
        emitInst.push_back(i);
        emitBase.push_back((uint32_t)total);
        instOffset[i] = (uint32_t)total;
        total += tris;
        if (total > SKH_EMIT_MAX_ENTRIES)
        {
            c->dev.err = "emitter table: more than 2^24 emissive triangles (SKH_EMIT_MAX_ENTRIES)";
            return SKH_INVALID_ARGUMENT;
        }
    }
    const uint32_t n = (uint32_t)total, nEmit = (uint32_t)emitInst.size();
    if (n == 0)
    {
        emit_clear(c);
        c->emit.msBuild = 0.0;
        c->emit.stale = false;
        return SKH_OK;
    }
    emitBase.push_back(n);
    uint32_t bits = 0;
    while ((1u << bits) < n)
        ++bits;
    const uint32_t G = 1u << bits, nTiles = (n + SKH_EMIT_TILE - 1u) / SKH_EMIT_TILE;
    DevBuf dEntries, dCdf, dGuide, dLe, dOff, dInst, dBase, dWeight, dTmp; // dTmp: the tile sums, sum w
    SKH_CHECK(dev_alloc(c, dEntries, (size_t)n * 4 * sizeof(float4)));
    SKH_CHECK(dev_alloc(c, dCdf, (size_t)n * sizeof(float)));
    SKH_CHECK(dev_alloc(c, dWeight, (size_t)n * sizeof(float)));
    SKH_CHECK(dev_alloc(c, dGuide, ((size_t)G + 1u) * sizeof(uint32_t)));
    SKH_CHECK(dev_alloc(c, dTmp, ((size_t)nTiles + 1u) * sizeof(double)));
    SKH_CHECK(dev_upload(c, dLe, le.data(), le.size() * sizeof(float)));
    SKH_CHECK(dev_upload(c, dOff, instOffset.data(), instOffset.size() * sizeof(uint32_t)));
    SKH_CHECK(dev_upload(c, dInst, emitInst.data(), emitInst.size() * sizeof(uint32_t)));
    SKH_CHECK(dev_upload(c, dBase, emitBase.data(), emitBase.size() * sizeof(uint32_t)));
    double* tileSum = dTmp.as<double>();
    double* sumW = tileSum + nTiles;
    hipStream_t st = c->dev.stream;
    k_emit_gather<<<(n + SKH_EMIT_BLOCK - 1u) / SKH_EMIT_BLOCK, SKH_EMIT_BLOCK, 0, st>>>(c->scene.dVerts.as<uint8_t>(), c->scene.dIndices.as<uint32_t>(), c->scene.dMeshes.as<uint4>(),
                                                                                       c->scene.dInstances.as<uint32_t>(), dLe.as<float4>(), nMat, dInst.as<uint32_t>(),
                                                                                       dBase.as<uint32_t>(), nEmit, n, dEntries.as<float4>(), dWeight.as<float>());
    k_emit_tile_sums<<<nTiles, SKH_EMIT_BLOCK, 0, st>>>(dWeight.as<float>(), n, tileSum);
    k_emit_scan_tiles<<<1, SKH_EMIT_BLOCK, 0, st>>>(tileSum, nTiles, sumW);
    k_emit_cdf<<<nTiles, SKH_EMIT_BLOCK, 0, st>>>(dWeight.as<float>(), n, tileSum, sumW, dCdf.as<float>());
    k_emit_guide<<<(G + 1u + SKH_EMIT_BLOCK - 1u) / SKH_EMIT_BLOCK, SKH_EMIT_BLOCK, 0, st>>>(dCdf.as<float>(), n, bits, dGuide.as<uint32_t>());
    SKH_TRY(c, hipGetLastError());
    double totalW = 0.0;
    SKH_TRY(c, hipMemcpyAsync(&totalW, sumW, sizeof(double), hipMemcpyDeviceToHost, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    c->emit.dEntries = std::move(dEntries), c->emit.dCdf = std::move(dCdf), c->emit.dGuide = std::move(dGuide), c->emit.dLe = std::move(dLe), c->emit.dInstOffset = std::move(dOff);
    c->emit.count = n, c->emit.instances = nEmit, c->emit.guideBits = bits;
    c->emit.sumW = totalW;
    c->emit.msBuild = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->emit.stale = false;
    return SKH_OK;
}

static EmitP make_emit(const skh_context* c)
{
    EmitP e;
    memset(&e, 0, sizeof(e));
    if (!(c->emit.sumW > 0.0))
        return e;
    e.entries = c->emit.dEntries.as<float4>();
    e.cdf = c->emit.dCdf.as<float>();
    e.guide = c->emit.dGuide.as<uint32_t>();
    e.Le = c->emit.dLe.as<float4>();
    e.instOffset = c->emit.dInstOffset.as<uint32_t>();
    e.count = c->emit.count, e.guideBits = c->emit.guideBits, e.numMaterials = std::max(1u, c->scene.nMaterials);
    e.nee = c->opt.emitNee;
    e.invSumW = (float)(1.0 / c->emit.sumW);
    return e;
}

skh_status skh_set_emission(skh_context* c, const float* rgb, uint32_t n)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (!rgb || n == 0)
    {
        // remove: a no-op on a context that has none (nothing traced ahead is thrown away for it)
        if (c->emit.emission.empty())
            return SKH_OK;
        spec_drop(c);
        c->emit.emission.clear();
        touched(c, skh_stale::IN_EMISSION);
        return SKH_OK;
    }
    if (n > c->scene.nMaterials)
    {
        c->dev.err = "skh_set_emission: " + std::to_string(n) + " radiances for " + std::to_string(c->scene.nMaterials) + " materials (call skh_set_materials first)";
        return SKH_INVALID_ARGUMENT;
    }
    for (size_t k = 0; k < 3 * (size_t)n; ++k)
        if (!(rgb[k] >= 0.0f) || std::isinf(rgb[k])) // (a NaN fails >=)
        {
            c->dev.err = "skh_set_emission: the radiances must be finite and >= 0";
            return SKH_INVALID_ARGUMENT;
        }
    spec_drop(c);
    bool any = false;
    for (size_t k = 0; k < 3 * (size_t)n; ++k)
        any = any || rgb[k] > 0.0f;
    if (any)
        c->emit.emission.assign(rgb, rgb + 3 * (size_t)n);
    else
        c->emit.emission.clear(); // (all black: the context of one that was never told)
    touched(c, skh_stale::IN_EMISSION);
    return SKH_OK;
}

skh_status skh_get_emitter_info(skh_context* c, skh_emitter_info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    (void)hipSetDevice(c->dev.device);
    SKH_CHECK(emit_ensure(c));
    out->triangles = c->emit.count, out->instances = c->emit.instances;
    out->sum_w = c->emit.sumW;
    out->ms_build = c->emit.msBuild;
    out->bytes = c->emit.count ? c->emit.dEntries.bytes + c->emit.dCdf.bytes + c->emit.dGuide.bytes + c->emit.dLe.bytes + c->emit.dInstOffset.bytes : 0u;
    return SKH_OK;
}

skh_status skh_emitter_probe(skh_context* c, uint32_t kind, const void* in, uint32_t n, void* out)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    if (kind > SKH_EMIT_PROBE_PDF || (n && (!in || !out)))
    {
        c->dev.err = "skh_emitter_probe: unknown kind, or a missing input / output pointer";
        return SKH_INVALID_ARGUMENT;
    }
    (void)hipSetDevice(c->dev.device);
    SKH_CHECK(emit_ensure(c));
    if (!(c->emit.sumW > 0.0))
    {
        c->dev.err = "skh_emitter_probe: the context has no emitter (no emissive material on a mesh instance)";
        return SKH_INVALID_ARGUMENT;
    }
    if (n == 0)
        return SKH_OK;
    const size_t inBytes = (kind == SKH_EMIT_PROBE_SAMPLE ? 6u : 8u) * sizeof(uint32_t), outBytes = (kind == SKH_EMIT_PROBE_SAMPLE ? 13u : 4u) * sizeof(uint32_t);
    // (Le at the sampled point carries the emission map: the uv comes from the shading records, which the build makes)
    const bool withMaps = kind == SKH_EMIT_PROBE_SAMPLE && mtex_active(c);
    if (withMaps)
        SKH_CHECK(ensure_ready(c));
    const ProbeIn pin[] = { { in, inBytes * n } };
    return probe_roundtrip(c, pin, out, outBytes * n, [&](const DevBuf* d, const DevBuf& dOut) {
        if (withMaps)
            k_emit_probe_mtex<<<(n + 255) / 256, 256, 0, c->dev.stream>>>(make_emit(c), make_mtex(c), make_dev_scene(c), d[0].as<float>(), n, dOut.as<uint32_t>());
        else
            k_emit_probe<<<(n + 255) / 256, 256, 0, c->dev.stream>>>(make_emit(c), (uint32_t)c->scene.instances.size(), kind, d[0].as<uint32_t>(), n, dOut.as<uint32_t>());
    });
}

static skh_status ensure_ready(skh_context* c)
{
    if (!c->accel.built)
    {
        skh_status s = skh_build_accel(c, SKH_BUILD_LBVH);
        if (s != SKH_OK)
            return s;
    }
    if (c->scene.nMaterials == 0)
    {
        // material 0 = default.mdl::default_material (OptixRender.cpp:1090-1097)
        skh_material m;
        memset(&m, 0, sizeof(m));
        m.type = SKH_MAT_DIFFUSE;
        m.base_color[0] = m.base_color[1] = m.base_color[2] = 0.8f;
        skh_status s = skh_set_materials(c, &m, 1);
        if (s != SKH_OK)
            return s;
    }
    SKH_CHECK(emit_ensure(c));
    SKH_CHECK(lshape_ensure(c));
    SKH_CHECK(cut_ensure(c));
    return cut_alloc_frame(c);
}

// ---- the trace launch ----
// The builds of k_trace a context can run; each exists for ANY x COUNT (no other combination of CURVES, WORLD and SPLIT is compiled).
enum TraceBuild
{
    TB_GENERAL,        // two-level, without the curve intersector (fewer VGPRs)
    TB_GENERAL_CURVES, // two-level with the curve intersector
    TB_WORLD,          // every instance is baked: the world-only build of the kernel (no instance entry, no object-space copy of the ray)
    TB_WORLD_SPLIT,    // ... whose tail phase hands stack entries to idle lanes (option tail_split)
    TB_WORLD_CURVES,   // the world-only kernel with the curve block: curve instances under identity transforms
    TB_COUNT
};
using TraceKernel = decltype(&k_trace<false, false, false>);
static const TraceKernel kTraceKernels[TB_COUNT][2 /* ANY */][2 /* COUNT */] = {
    { { k_trace<false, false, false>, k_trace<false, true, false> }, { k_trace<true, false, false>, k_trace<true, true, false> } },
    { { k_trace<false, false, true>, k_trace<false, true, true> }, { k_trace<true, false, true>, k_trace<true, true, true> } },
    { { k_trace<false, false, false, true>, k_trace<false, true, false, true> }, { k_trace<true, false, false, true>, k_trace<true, true, false, true> } },
    { { k_trace<false, false, false, true, true>, k_trace<false, true, false, true, true> }, { k_trace<true, false, false, true, true>, k_trace<true, true, false, true, true> } },
    { { k_trace<false, false, true, true>, k_trace<false, true, true, true> }, { k_trace<true, false, true, true>, k_trace<true, true, true, true> } },
};

// The build this context's launches run.  `split`: the pass asks for the SPLIT build (tail_split -1: render_one).
static TraceBuild trace_build(const skh_context* c, bool split)
{
    const bool noTopLevel = c->accel.tlasRoot == SKH_REF_INVALID && c->opt.worldKernel;
    if (!c->accel.nSegs && noTopLevel && (c->accel.worldRoot != SKH_REF_INVALID || c->accel.lightRoot != SKH_REF_INVALID))
        return (c->opt.tailSplit == 2 || (c->opt.tailSplit == 1 && c->accel.hierNodes > 16384u) || split) ? TB_WORLD_SPLIT : TB_WORLD;
    if (c->accel.nSegs && noTopLevel && c->accel.numWorldCurves > 0)
        return TB_WORLD_CURVES;
    // scenes without curve instances run the build of the kernel that has no curve intersector in it (fewer VGPRs)
    return c->accel.nSegs ? TB_GENERAL_CURVES : TB_GENERAL;
}

// Everything one launch of the persistent trace kernel depends on beside the scene and the context's options.
struct TraceLaunch
{
    RayQ rq;                // the queue,
    const uint32_t* counts; // its length words
    uint32_t* fetch;        // and its 8 fetch cursors, zeroed
    HitQ hq;
    PathS ps;
    const float4* contrib; // any-hit launches of a render pass: the shadow rays' contributions
    hipStream_t stream;
    bool any;
    uint32_t smallGrid; // an overlapped small pass: this launch's share of the machine, waves per (32-wave) CU x CUs; 0 = the build's full grid
    bool split;         // the SPLIT build for this pass (trace_build)
};

// one launch of the persistent trace kernel over a sharded queue: picks the build and the grid
static void launch_trace(skh_context* c, const DevScene& sc, const TraceLaunch& t)
{
    const bool any = t.any;
    const TraceBuild build = trace_build(c, t.split);
    const bool curveBuild = c->accel.nSegs != 0;
    // (small overlapped passes, triangle scenes: a closest-hit wave asks for rays when 48 instead of 32 of its lanes are idle -- 1-spp 1080p call 3.11 -> 3.01 ms; 40 / 56: 3.04 / 3.04; lower
    // thresholds lose: 24 / 16 / 8: 3.20 / 3.29 / 3.44; the any-hit threshold stays: 32 / 56 of 64: 3.16 / 3.12 against 3.11 at 48.  An explicit fetch_min_closest applies everywhere.)
    const uint32_t fetchMinClosest = (t.smallGrid && !curveBuild && !c->opt.fetchMinClosestSet) ? c->opt.fetchMinClosestSmall : (curveBuild ? c->opt.curveFetchMinClosest : c->opt.fetchMinClosest);
    const uint32_t fetchMin = any ? (curveBuild ? c->opt.curveFetchMinShadow : c->opt.fetchMinShadow) : fetchMinClosest;
    const uint32_t nodeBreak = any ? (curveBuild ? c->opt.curveNodeBreakShadow : c->opt.nodeBreakShadow) : (curveBuild ? c->opt.curveNodeBreakClosest : c->opt.nodeBreakClosest);
    // (the world-only kernel with the curve block -- curve instances under identity transforms -- wants the triangle kernels' node-loop exits and
    // an earlier curve block: hair stand-in 1 862 -> 1 937 Mray/s with 32 / 28 / 32 against the two-level curve build's 20 / 20 / 48, gpurun_out/r5t)
    const bool worldCurves = build == TB_WORLD_CURVES;
    const uint32_t nodeBreakW = worldCurves ? (any ? c->opt.nodeBreakShadow : c->opt.nodeBreakClosest) : nodeBreak;
    const uint32_t fm = fetchMin | ((worldCurves ? c->opt.worldCurveMin : c->opt.curveMin) << 8) | (nodeBreakW << 16) | (c->opt.leafMin << 24);
    hipStream_t st = t.stream;
    int* ovf = st == c->dev.stream ? c->frame.dOvf.as<int>() : c->frame.dOvf2.as<int>(); // (two trace kernels may be in flight)
    StatsDev* sd = c->timing.dStats.as<StatsDev>();
    const bool worldOnly = build == TB_WORLD || build == TB_WORLD_SPLIT;
    // (the world-only triangle builds run 8 waves per SIMD)
    const uint32_t fullGrid = (any && !c->accel.nSegs) ? (uint32_t)c->dev.numCUs * (worldOnly ? c->opt.wavesPerCUShadowWorld : c->opt.wavesPerCUShadow)
                                                 : (worldOnly ? (uint32_t)c->dev.numCUs * c->opt.wavesPerCUWorld : c->frame.traceBlocks);
    // (overlapped small passes: small_waves_* are shares of a 32-wave CU; a build that fits fewer waves -- the curve builds: 24 -- takes the same share of what it fits,
    // so that the two concurrent launches still fit side by side: hair 1-spp calls 651 -> ~680 Mray/s against an unscaled 20 / 12)
    const uint32_t scaledGrid = (uint32_t)((uint64_t)t.smallGrid * fullGrid / (32u * (uint32_t)c->dev.numCUs));
    const uint32_t blocks = t.smallGrid ? std::max((uint32_t)c->dev.numCUs, std::min(scaledGrid, fullGrid)) : fullGrid;
    // A hierarchy that fits the L2 many times over (Cornell: 30 triangles) makes rays so cheap that the launch is bound by the eight queue cursors'
    // atomics (~88 M per second and address): such scenes reserve 128 positions per atomic (Cornell 13.5 -> 14.8 Gray/s).  Larger scenes lose by it
    // (neighbouring rays are then traced at different times by one wave instead of together by neighbouring waves: kitchen -1 %, hair -2 %;
    // docs/LOG.md, round 5); only the world-only triangle builds carry the code.
    const uint32_t chunk = c->opt.fetchChunk >= 0 ? (uint32_t)c->opt.fetchChunk : (c->accel.hierNodes <= 16384u ? 128u : 0u);
#ifdef SKH_TAIL_PROFILE
    (void)hipMemsetAsync(&sd->launchT0[any ? 1 : 0], 0xff, sizeof(unsigned long long), st);
#endif
    kTraceKernels[build][any ? 1 : 0][c->opt.countTraversal ? 1 : 0]<<<blocks, SKH_TRACE_BLOCK, 0, st>>>(sc, t.rq, t.counts, t.fetch, fm, t.hq, t.ps, t.contrib, ovf, sd, c->accel.lightBox, chunk);
}

// what the closest-hit launches of SHADOW rays walk: not the baked light proxies' tree (shadow rays do not see lights)
static DevScene shadow_scene(const skh_context* c, DevScene sc)
{
    if (c->accel.worldRoot != SKH_REF_INVALID || c->accel.tlasRoot != SKH_REF_INVALID)
        sc.lightRoot = SKH_REF_INVALID;
    return sc;
}

// what the cutout rounds behind a trace launch work in: two continuation queues, a second hit buffer, cutout_rounds x SKH_CUT_WORDS zeroed words
struct CutRounds
{
    RayQ q[2];
    HitQ h0, h2;   // h0: where a SHADOW step's first launch leaves its nearest hits (a closest step's lie where the caller wants them)
    float* rawOut; // raw shadow queries: one float per ray
    uint32_t* words;
    uint32_t rays;
    BlendP bl;
};
static const decltype(&k_cutout<false, false>) kCutoutKernels[2 /* SHADOW */][2 /* BLEND */] = { { k_cutout<false, false>, k_cutout<false, true> },
                                                                                                  { k_cutout<true, false>, k_cutout<true, true> } };

// The continuation rounds behind the trace launch `t`, whose hit records lie in t.hq: k_cutout on them, then cutout_rounds x {trace the continuation queue into h2,
// k_cutout}; those launches take t's stream, grid share and split flag.  A round whose queue is empty costs two launches that return at once.
static void run_cutout_chain(skh_context* c, const DevScene& sc, const DevScene& scTrace, const TraceLaunch& t, bool shadow, const float4* contrib, const CutRounds& cr)
{
    const CutoutP cutp = make_cutout(c);
    // the BLEND build only where blending is in use (bl.count != 0: make_blend); round = hits the rays of a launch have already passed; the path ids lie in the first queue
    BlendP bl = cr.bl;
    const auto kernel = kCutoutKernels[shadow ? 1 : 0][bl.count != 0u ? 1 : 0];
    bl.pathIds = reinterpret_cast<const uint32_t*>(t.rq.base + (size_t)8 * t.rq.stride);
    CutStatsDev* cst = c->cut.dStats.as<CutStatsDev>();
    const uint32_t perShard = (((cr.rays + SKH_SHARDS - 1u) / SKH_SHARDS) + 63u) & ~63u;
    const dim3 grid(SKH_SHARDS * ((std::min(perShard, t.rq.region) + SKH_CUTOUT_BLOCK - 1) / SKH_CUTOUT_BLOCK));
    const uint32_t R = c->opt.cutoutRounds, QW = SKH_COUNT_STRIDE * SKH_SHARDS;
    bl.round = 0u;
    kernel<<<grid, SKH_CUTOUT_BLOCK, 0, t.stream>>>(sc, cutp, t.rq, t.counts, t.hq, 1u, 0u, t.hq, cr.rawOut, t.ps, contrib, cr.q[0], cr.words, cst, bl);
    TraceLaunch next = t; // (any = false, contrib = nullptr: trace_step)
    next.hq = cr.h2;
    for (uint32_t r = 0; r < R; ++r)
    {
        uint32_t* lens = cr.words + (size_t)r * SKH_CUT_WORDS;
        next.rq = cr.q[r & 1], next.counts = lens, next.fetch = lens + QW;
        launch_trace(c, scTrace, next);
        const bool last = r + 1 == R;
        bl.round = r + 1u;
        kernel<<<grid, SKH_CUTOUT_BLOCK, 0, t.stream>>>(sc, cutp, next.rq, lens, cr.h2, 0u, last ? 1u : 0u, t.hq, cr.rawOut, t.ps, contrib, cr.q[(r + 1) & 1],
                                                        last ? lens : lens + SKH_CUT_WORDS, cst, bl);
    }
}

// One trace step of a pass or of a raw query.  Without the cutout stage (cr == nullptr) it is the launch: any-hit for shadow rays.  With it, the nearest hits are
// wanted: a closest-hit launch -- a shadow step's into cr->h0, past the light proxies -- and the rounds behind it, which add a shadow ray's contribution when it ends in a miss.
static void trace_step(skh_context* c, const DevScene& sc, TraceLaunch t, bool shadow, const CutRounds* cr)
{
    t.any = shadow && !cr;
    if (!cr)
        return launch_trace(c, sc, t);
    const float4* contrib = t.contrib;
    t.contrib = nullptr;
    if (shadow)
        t.hq = cr->h0;
    const DevScene scTrace = shadow ? shadow_scene(c, sc) : sc;
    launch_trace(c, scTrace, t);
    run_cutout_chain(c, sc, scTrace, t, shadow, contrib, *cr);
}

// After a synchronisation: did any traversal of the calls since the last check drop a stack entry (its result may miss hits)?
static skh_status check_stack_overflow(skh_context* c, const char* where)
{
    if (!*c->dev.hOverflow)
        return SKH_OK;
    *c->dev.hOverflow = 0u;
    c->timing.stackOverflows++;
    c->dev.err = std::string(where) + ": a traversal stack overflowed its " + std::to_string(SKH_STACK_LDS) + " LDS + " + std::to_string(SKH_STACK_OVF) +
             " global entries and dropped a subtree: hits may be missing (degenerate hierarchy?)";
    return SKH_FAIL;
}

// ---- adaptive sampling (skh_adapt.h) ----
static_assert(sizeof(skh_adaptive) == 32 && sizeof(skh_adaptive_info) == 40, "ABI layout");

skh_status skh_adaptive_check(const skh_adaptive* a)
{
    if (!a || !std::isfinite(a->threshold) || a->threshold < 0.0f || !std::isfinite(a->dark_level) || !(a->dark_level > 0.0f) || a->min_samples < 2u ||
        a->interval < 1u || a->reserved[0] || a->reserved[1] || a->reserved[2] || a->reserved[3])
        return SKH_INVALID_ARGUMENT;
    return SKH_OK;
}

skh_status skh_set_adaptive(skh_context* c, const skh_adaptive* a)
{
    if (!c || (a && skh_adaptive_check(a) != SKH_OK))
    {
        if (c)
            c->dev.err = "skh_set_adaptive: threshold finite and >= 0, dark_level finite and > 0, min_samples >= 2, interval >= 1, reserved words 0";
        return SKH_INVALID_ARGUMENT;
    }
    (void)hipSetDevice(c->dev.device);
    spec_drop(c); // (also: the adaptive frame starts again)
    c->adapt.on = a != nullptr;
    if (a)
        c->adapt.cfg = *a;
    else
    {
        SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
        c->adapt = skh_context::Adaptive(); // (frees the feature's five buffers)
    }
    return SKH_OK;
}

// whether this call is an adaptive one
static inline bool adapt_applies(const skh_context* c, const skh_frame_params& p)
{
    return c->adapt.on && p.enable_accumulation != 0 && p.debug == 0;
}

// Before the first pass of an adaptive call: where the frame starts (sub-frame 0, or a reset since the last call) every tile becomes active and the statistics are
// cleared -- the render list and its tables are the home list's again.  The accumulators need nothing: sub-frame 0 overwrites them.
static skh_status adapt_prepare(skh_context* c, const skh_frame_params& p)
{
    skh_context::Adaptive& ad = c->adapt;
    if (ad.ready && p.subframe_index != 0)
        return SKH_OK;
    const size_t N1 = std::max(1u, c->frame.numSlots), nt = std::max(1u, c->frame.numTiles);
    const size_t baseBytes = sizeof(uint32_t) * std::max(1u, c->frame.raygenBlocksPerSub);
    SKH_CHECK(dev_alloc(c, c->adapt.dTileXYRender, sizeof(uint32_t) * 2 * nt));
    SKH_CHECK(dev_alloc(c, c->adapt.dRaygenBaseRender, baseBytes));
    SKH_CHECK(dev_alloc(c, c->adapt.dState, sizeof(float4) * N1));
    SKH_CHECK(dev_alloc(c, c->adapt.dTileQ, sizeof(float) * nt));
    SKH_CHECK(dev_alloc(c, c->adapt.dFrozenAt, sizeof(uint32_t) * nt));
    SKH_TRY(c, hipMemcpyAsync(c->adapt.dTileXYRender.p, c->frame.dTileXY.p, sizeof(uint32_t) * 2 * c->frame.numTiles, hipMemcpyDeviceToDevice, c->dev.stream));
    SKH_TRY(c, hipMemcpyAsync(c->adapt.dRaygenBaseRender.p, c->frame.dRaygenBase.p, baseBytes, hipMemcpyDeviceToDevice, c->dev.stream));
    SKH_TRY(c, hipMemsetAsync(c->adapt.dState.p, 0, sizeof(float4) * N1, c->dev.stream));
    SKH_TRY(c, hipMemsetAsync(c->adapt.dTileQ.p, 0, sizeof(float) * nt, c->dev.stream));
    SKH_TRY(c, hipMemsetAsync(c->adapt.dFrozenAt.p, 0, sizeof(uint32_t) * nt, c->dev.stream));
    ad.frozenAt.assign(c->frame.numTiles, 0u);
    ad.delivered = ad.checks = 0;
    ad.activeTiles = c->frame.numTiles;
    ad.raygenValid = c->frame.raygenValidPerSub;
    ad.orderGen++; // (the cell order's tables of the last frame's frozen sets are stale)
    ad.pixelObs = ad.pixelObsSaved = 0;
    ad.ready = true;
    return SKH_OK;
}

// launches until the next check, with `delivered` observations made (>= 1)
static inline uint32_t adapt_to_next_check(const skh_context* c)
{
    const skh_context::Adaptive& ad = c->adapt;
    if (ad.delivered < ad.cfg.min_samples)
        return ad.cfg.min_samples - ad.delivered;
    return ad.cfg.interval - (ad.delivered - ad.cfg.min_samples) % ad.cfg.interval;
}

// the fields of FrameP that describe the frame's geometry
static void frame_geometry(const skh_context* c, FrameP& fp)
{
    fp.width = c->frame.width, fp.height = c->frame.height, fp.tileSize = c->frame.tileSize, fp.tileShift = c->frame.tileShift, fp.numTiles = c->frame.numTiles, fp.numSlots = c->frame.numSlots;
}

static FrameP adapt_frame(const skh_context* c, const skh_frame_params& p)
{
    FrameP fp;
    memset(&fp, 0, sizeof(fp));
    memcpy(fp.exposure, p.exposure, sizeof(fp.exposure));
    frame_geometry(c, fp);
    return fp;
}

// After a pass of `launches` observations: count them, and where their number is one at which a check happens, run it: the decision kernel, the flags back (one word
// per tile), and -- when a tile froze -- the ray-generation tables of the new render list up (the kernel has moved the origins in the device's list itself).
static skh_status adapt_after_pass(skh_context* c, const skh_frame_params& p, uint32_t launches)
{
    skh_context::Adaptive& ad = c->adapt;
    ad.delivered += launches;
    ad.pixelObs += (uint64_t)ad.raygenValid * launches;
    ad.pixelObsSaved += (uint64_t)(c->frame.raygenValidPerSub - ad.raygenValid) * launches;
    if (ad.delivered < ad.cfg.min_samples || (ad.delivered - ad.cfg.min_samples) % ad.cfg.interval != 0u || c->frame.numTiles == 0u)
        return SKH_OK;
    const float thr2 = ad.cfg.threshold * ad.cfg.threshold;
    {
        SpanGuard g(c, KC_ACCUM);
        k_adapt_tiles<<<c->frame.numTiles, 256, 0, c->dev.stream>>>(adapt_frame(c, p), c->adapt.dTileXYRender.as<uint32_t>(), c->adapt.dState.as<float4>(), ad.delivered, thr2,
                                                          ad.cfg.dark_level, c->adapt.dTileQ.as<float>(), c->adapt.dFrozenAt.as<uint32_t>());
    }
    ad.checks++;
    SKH_TRY(c, hipMemcpyAsync(ad.frozenAt.data(), c->adapt.dFrozenAt.p, sizeof(uint32_t) * c->frame.numTiles, hipMemcpyDeviceToHost, c->dev.stream));
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    uint32_t active = 0;
    for (uint32_t t = 0; t < c->frame.numTiles; ++t)
        active += ad.frozenAt[t] == 0u ? 1u : 0u;
    if (active != ad.activeTiles)
    {
        std::vector<uint32_t> base;
        raygen_tables(c, ad.frozenAt.data(), base, ad.raygenValid);
        SKH_TRY(c, hipMemcpyAsync(c->adapt.dRaygenBaseRender.p, base.data(), sizeof(uint32_t) * base.size(), hipMemcpyHostToDevice, c->dev.stream));
        SKH_TRY(c, hipStreamSynchronize(c->dev.stream)); // (`base` goes out of scope)
        ad.activeTiles = active;
        ad.orderGen++; // (... and the cell order's, which the next pass builds when it needs them: raygen_order)
    }
    return SKH_OK;
}

// the frozen tiles' pixels of a call's d_image
static void adapt_fill(skh_context* c, const skh_frame_params& p, void* d_image)
{
    if (!d_image || c->adapt.activeTiles == c->frame.numTiles || c->frame.numSlots == 0u)
        return;
    SpanGuard g(c, KC_ACCUM);
    k_adapt_fill<<<(c->frame.numSlots + 255) / 256, 256, 0, c->dev.stream>>>(adapt_frame(c, p), c->frame.dTileXY.as<uint32_t>(), c->adapt.dFrozenAt.as<uint32_t>(),
                                                                 c->frame.dAccum.as<float4>(), reinterpret_cast<float4*>(d_image));
}

skh_status skh_get_adaptive_info(skh_context* c, skh_adaptive_info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    const skh_context::Adaptive& ad = c->adapt;
    memset(out, 0, sizeof(*out));
    out->enabled = ad.on ? 1u : 0u;
    out->tiles = c->frame.numTiles;
    out->active_tiles = c->frame.numTiles;
    if (!ad.on || !ad.ready)
        return SKH_OK; // (the frame has not begun: every tile active, nothing observed)
    out->active_tiles = ad.activeTiles;
    out->checks = ad.checks;
    uint32_t lo = 0xffffffffu, hi = 0;
    for (uint32_t t = 0; t < c->frame.numTiles; ++t)
    {
        const uint32_t n = ad.frozenAt[t] ? ad.frozenAt[t] : ad.delivered;
        lo = std::min(lo, n), hi = std::max(hi, n);
    }
    out->min_observations = c->frame.numTiles ? lo : 0u;
    out->max_observations = hi;
    out->pixel_observations = ad.pixelObs;
    out->pixel_observations_saved = ad.pixelObsSaved;
    return SKH_OK;
}

// What one call of render_one does.  One wavefront pass: either one launch of p->samples_this_launch samples (batch = 1), or `batch` consecutive sub-frames
// of one sample each traced together (more rays per launch; results identical, see k_finalize_batch).
struct RenderPlan
{
    uint32_t batch = 1;
    bool trace = true;                                 // false: the pass was traced ahead, only accumulation steps are left
    uint32_t finalFirst = 0, finalCount = 0xffffffffu; // the sub-frames of the pass whose accumulation steps this call applies
    uint32_t pathSel = 0;                              // 1: the second path-state buffer
    bool finalize = true;
    hipStream_t finStream = nullptr; // where the accumulation step runs (default: the render stream)
    bool adaptive = false;           // an adaptive pass: the render list and its tables -- frozen tiles are slots outside the image to every kernel
};

// what the steps of a pass share
struct RenderPass
{
    FrameP fp;
    DevScene sc;
    EnvP envp;
    EmitP emitp;
    MtexP mtexp;
    LshapeP lshp;
    hipStream_t st;
    const uint32_t* tiles;
    PathS ps;
    RayQ rq[2], shq, cutQ[2], cutSQ[2];
    HitQ hq, cutH, cutSH0, cutSH1;
    uint32_t *counts, *fetch, *cutWords;
    uint32_t QW, NP, rounds, cutBounceWords;
    bool smallPass, useOverlap, split, cutOn;
    BlendP blp;
};

static FrameP frame_params(const skh_context* c, const skh_frame_params* p, const RenderPlan& plan)
{
    FrameP fp;
    memcpy(fp.viewToWorld, p->view_to_world, sizeof(fp.viewToWorld));
    memcpy(fp.clipToView, p->clip_to_view, sizeof(fp.clipToView));
    fp.subframeIndex = p->subframe_index;
    fp.samplesThisLaunch = p->samples_this_launch;
    fp.sppTotal = p->spp_total;
    fp.maxDepth = p->max_depth;
    fp.rectMethod = p->rect_light_sampling_method;
    memcpy(fp.exposure, p->exposure, sizeof(fp.exposure));
    fp.enableAccumulation = p->enable_accumulation;
    fp.debug = p->debug;
    fp.shadowTmin = p->shadow_ray_tmin;
    fp.materialTmin = p->material_ray_tmin;
    frame_geometry(c, fp);
    fp.batch = plan.batch;
    fp.finalFirst = std::min(plan.finalFirst, plan.batch);
    fp.finalCount = std::min(plan.finalCount, plan.batch - fp.finalFirst);
    return fp;
}

// tmin / tmax of every radiance ray and tmin of every shadow ray are constants of the frame parameters (OptixRender.cu:121-122, closest_hit.cu):
// their queue planes are filled here, when the queues are new or a value has changed, and never written per ray (8 + 8 + 4 B per path and bounce)
static void fill_queue_constants(skh_context* c, const RenderPass& rp)
{
    const uint32_t NQ = rp.shq.stride;
    uint32_t bits[2];
    memcpy(&bits[0], &rp.fp.materialTmin, 4);
    memcpy(&bits[1], &rp.fp.shadowTmin, 4);
    if (c->frame.queueConstFilled && bits[0] == c->frame.queueConstBits[0] && bits[1] == c->frame.queueConstBits[1])
        return;
    const uint32_t fb = (uint32_t)c->dev.numCUs * 8u;
    for (int k = 0; k < 2; ++k)
    {
        k_fill_f32<<<fb, 256, 0, rp.st>>>(rp.rq[k].base + (size_t)6 * NQ, NQ, rp.fp.materialTmin);
        k_fill_f32<<<fb, 256, 0, rp.st>>>(rp.rq[k].base + (size_t)7 * NQ, NQ, 1e16f);
    }
    k_fill_f32<<<fb, 256, 0, rp.st>>>(rp.shq.base + (size_t)6 * NQ, NQ, rp.fp.shadowTmin);
    c->frame.queueConstFilled = true;
    c->frame.queueConstBits[0] = bits[0];
    c->frame.queueConstBits[1] = bits[1];
}

// k_shade for bounce b of sample s: the build by HAIR x ENV x EMIT x MTEX (index 8 4 2 1) and by the bounce's position (SHADE_FIRST / MIDDLE / LAST, skh_kernels.h);
// every one has a twin with light shapes in it, launched only when a shape is in use.  -DSKH_SHADE_POSITIONS=0: one build per flag combination, for every bounce.
#define SKH_SHADE_BUILDS(K, P)                                                                                                                               \
    {                                                                                                                                                        \
        K<false, false, false, false, P>, K<false, false, false, true, P>, K<false, false, true, false, P>, K<false, false, true, true, P>,                  \
        K<false, true, false, false, P>, K<false, true, false, true, P>, K<false, true, true, false, P>, K<false, true, true, true, P>,                      \
        K<true, false, false, false, P>, K<true, false, false, true, P>, K<true, false, true, false, P>, K<true, false, true, true, P>,                      \
        K<true, true, false, false, P>, K<true, true, false, true, P>, K<true, true, true, false, P>, K<true, true, true, true, P>                           \
    }
#if SKH_SHADE_POSITIONS
#define SKH_SHADE_TABLE(K) { SKH_SHADE_BUILDS(K, SHADE_FIRST), SKH_SHADE_BUILDS(K, SHADE_MIDDLE), SKH_SHADE_BUILDS(K, SHADE_LAST) }
#else
#define SKH_SHADE_TABLE(K) { SKH_SHADE_BUILDS(K, SHADE_ANY), SKH_SHADE_BUILDS(K, SHADE_ANY), SKH_SHADE_BUILDS(K, SHADE_ANY) }
#endif
static const decltype(&k_shade<false, false, false, false, SHADE_ANY>) kShadeKernels[3][16] = SKH_SHADE_TABLE(k_shade);
static const decltype(&k_shade_lshape<false, false, false, false, SHADE_ANY>) kShadeLshapeKernels[3][16] = SKH_SHADE_TABLE(k_shade_lshape);
#undef SKH_SHADE_TABLE
#undef SKH_SHADE_BUILDS

static void launch_shade(skh_context* c, const RenderPass& rp, uint32_t s, uint32_t b)
{
    // a shard holds at most an eighth of the pass's paths (rounded up to whole waves): SKH_SHARDS x that many workgroups,
    // workgroup b on shard b & 7; those past the end of their shard leave at once
    const uint32_t perShard = (((rp.NP + SKH_SHARDS - 1u) / SKH_SHARDS) + 63u) & ~63u;
    const dim3 sg(SKH_SHARDS * ((perShard + SKH_SHADE_BLOCK - 1) / SKH_SHADE_BLOCK));
    const uint32_t build = (c->scene.hasHairMaterial ? 8u : 0u) | (c->env.w ? 4u : 0u) | (rp.emitp.count ? 2u : 0u) | (rp.mtexp.count ? 1u : 0u), QW = rp.QW;
    uint32_t* counts = rp.counts;
    // bounce 0 runs the FIRST build whatever max_depth is (max_depth 1: its runtime depth test ends the paths); the last of several bounces the LAST build
    const uint32_t pos = b == 0u ? 0u : b + 1u == rp.rounds ? 2u : 1u;
    if (rp.lshp.table)
        kShadeLshapeKernels[pos][build]<<<sg, SKH_SHADE_BLOCK, 0, rp.st>>>(rp.sc, rp.fp, s, b, rp.tiles, rp.rq[b & 1], counts + 2 * b * QW, rp.hq, rp.ps, rp.rq[(b + 1) & 1],
                                                                      counts + 2 * (b + 1) * QW, rp.shq, c->frame.dContrib.as<float4>(), counts + (2 * b + 1) * QW, rp.envp,
                                                                      rp.emitp, rp.mtexp, rp.lshp);
    else
        kShadeKernels[pos][build]<<<sg, SKH_SHADE_BLOCK, 0, rp.st>>>(rp.sc, rp.fp, s, b, rp.tiles, rp.rq[b & 1], counts + 2 * b * QW, rp.hq, rp.ps, rp.rq[(b + 1) & 1],
                                                                counts + 2 * (b + 1) * QW, rp.shq, c->frame.dContrib.as<float4>(), counts + (2 * b + 1) * QW, rp.envp, rp.emitp,
                                                                rp.mtexp);
}

// Bounce b of sample s: the closest-hit step, k_shade, the shadow step.  With `overlap`, shadow[b] runs on a second stream: it depends on shade[b] only, and so does
// closest[b+1]; each fills the other's tail.
static void render_bounce(skh_context* c, const RenderPass& rp, uint32_t s, uint32_t b)
{
    hipStream_t st = rp.st;
    const bool smallGrids = rp.useOverlap && rp.smallPass;
    BlendP blp = rp.blp;
    blp.depth = b;
    uint32_t* words = rp.cutOn ? rp.cutWords + (size_t)b * rp.cutBounceWords : nullptr; // this bounce's: the closest side's, then the shadow side's
    TraceLaunch t;
    t.ps = rp.ps, t.split = rp.split, t.any = false;
    {
        SpanGuard g(c, KC_TRACE_CLOSEST);
        t.rq = rp.rq[b & 1], t.counts = rp.counts + 2 * b * rp.QW, t.fetch = rp.fetch + 16 * b * SKH_FETCH_STRIDE, t.hq = rp.hq, t.contrib = nullptr, t.stream = st;
        t.smallGrid = smallGrids ? ((b == 0 && c->opt.smallWavesFirst) ? c->opt.smallWavesFirst : c->opt.smallWavesClosest ? c->opt.smallWavesClosest : (c->accel.nSegs ? 16u : 20u)) * (uint32_t)c->dev.numCUs : 0u;
        const CutRounds cr{ { rp.cutQ[0], rp.cutQ[1] }, rp.hq, rp.cutH, nullptr, words, rp.NP, blp };
        trace_step(c, rp.sc, t, false, rp.cutOn ? &cr : nullptr);
    }
    if (rp.useOverlap && b > 0)
        (void)hipStreamWaitEvent(st, c->dev.evShadow, 0); // shade[b] reads the radiance shadow[b-1] adds to and reuses its queue
    {
        SpanGuard g(c, KC_SHADE);
        launch_shade(c, rp, s, b);
    }
    hipStream_t sst = rp.useOverlap ? c->dev.stream2 : st;
    if (rp.useOverlap)
    {
        (void)hipEventRecord(c->dev.evShade, st);
        (void)hipStreamWaitEvent(sst, c->dev.evShade, 0);
    }
    {
        SpanGuard g(c, KC_TRACE_SHADOW, sst);
        t.rq = rp.shq, t.counts = rp.counts + (2 * b + 1) * rp.QW, t.fetch = rp.fetch + (16 * b + 8) * SKH_FETCH_STRIDE, t.hq = HitQ{ nullptr, 0 }, t.contrib = c->frame.dContrib.as<float4>(), t.stream = sst;
        t.smallGrid = smallGrids ? ((b + 1 == rp.rounds && (c->opt.smallWavesLast || (!c->opt.smallWavesShadow && !c->accel.nSegs))) ? (c->opt.smallWavesLast ? c->opt.smallWavesLast : 20u) : c->opt.smallWavesShadow ? c->opt.smallWavesShadow : (c->accel.nSegs ? 16u : 12u)) * (uint32_t)c->dev.numCUs : 0u;
        // (a cutout in use) the shadow rays' NEAREST hits, tested and continued like the radiance rays'; a ray that ends in a miss adds its contribution (k_cutout)
        const CutRounds cr{ { rp.cutSQ[0], rp.cutSQ[1] }, rp.cutSH0, rp.cutSH1, nullptr, rp.cutOn ? words + c->opt.cutoutRounds * SKH_CUT_WORDS : nullptr, rp.NP, blp };
        trace_step(c, rp.sc, t, true, rp.cutOn ? &cr : nullptr);
    }
    if (rp.useOverlap)
        (void)hipEventRecord(c->dev.evShadow, sst);
}

// the accumulation steps of a pass into the frame's accumulators (and the call's d_image)
static void render_accumulate(skh_context* c, const RenderPass& rp, const RenderPlan& plan, bool oneSampleDirect, void* d_image)
{
    if (!plan.finalize)
        return;
    const uint32_t gridSlots = (c->frame.numSlots + 255) / 256;
    const bool fromPaths = plan.batch > 1 || oneSampleDirect;
    hipStream_t fs = plan.finStream ? plan.finStream : rp.st;
    {
        SpanGuard g(c, KC_ACCUM, fs);
        if (fromPaths)
            k_finalize_batch<<<gridSlots, 256, 0, fs>>>(rp.fp, rp.tiles, rp.ps, c->frame.dAccum.as<float4>(), c->frame.dDiffuse.as<float4>(), c->frame.dSpecular.as<float4>(),
                                                        c->frame.dDiffCnt.as<uint16_t>(), c->frame.dSpecCnt.as<uint16_t>(), reinterpret_cast<float4*>(d_image));
        else
            k_finalize<<<gridSlots, 256, 0, fs>>>(rp.fp, rp.tiles, c->frame.dSums.as<float>(), c->frame.dAccum.as<float4>(), c->frame.dDiffuse.as<float4>(), c->frame.dSpecular.as<float4>(),
                                                  c->frame.dDiffCnt.as<uint16_t>(), c->frame.dSpecCnt.as<uint16_t>(), reinterpret_cast<float4*>(d_image));
    }
    if (plan.adaptive)
    {
        SpanGuard g(c, KC_ACCUM, fs);
        k_adapt_moments<<<gridSlots, 256, 0, fs>>>(rp.fp, rp.tiles, rp.ps, c->frame.dSums.as<float>(), fromPaths ? 0u : 1u, c->adapt.dState.as<float4>());
    }
}

static skh_status render_one(skh_context* c, const skh_frame_params* p, const RenderPlan& plan, void* d_image)
{
    if (p->max_depth > 128 || p->samples_this_launch == 0)
    {
        c->dev.err = "skh_render_subframe: max_depth must be <= 128 (MAX_BOUNCES, RandomSampler.h:35) and samples_this_launch >= 1";
        return SKH_INVALID_ARGUMENT;
    }
    RenderPass rp;
    hipStream_t st = rp.st = c->dev.stream;
    const FrameP& fp = rp.fp = frame_params(c, p, plan);
    const uint32_t batch = plan.batch;
    rp.sc = make_dev_scene(c);
    rp.envp = make_env(c);
    rp.emitp = make_emit(c);
    rp.mtexp = make_mtex(c);
    rp.lshp = make_lshape(c);
    const uint32_t N = c->frame.numSlots * c->frame.batchCapacity; // plane stride of the path-state buffer
    const uint32_t NQ = SKH_SHARDS * c->frame.queueRegion; // plane stride of every queue (rays, hits, shadow contributions)
    const uint32_t NP = rp.NP = c->frame.numSlots * batch; // paths in this pass
    if (NP == 0)
        return SKH_OK;
    rp.tiles = plan.adaptive ? c->adapt.dTileXYRender.as<uint32_t>() : c->frame.dTileXY.as<uint32_t>();
    RaygenOrder order;
    if (plan.trace)
        SKH_CHECK(raygen_order(c, plan.adaptive, batch, order));
    const uint32_t raygenValid = plan.adaptive ? c->adapt.raygenValid : c->frame.raygenValidPerSub;
    rp.ps = PathS{ plan.pathSel ? c->spec.dPathB.as<float>() : c->frame.dPath.as<float>(), plan.pathSel ? c->spec.pathBStride : N };
    const auto queue = [&](const DevBuf& b) { return RayQ{ b.as<float>(), NQ, c->frame.queueRegion }; };
    rp.rq[0] = queue(c->frame.dRayQ[0]), rp.rq[1] = queue(c->frame.dRayQ[1]), rp.shq = queue(c->frame.dShadowQ);
    HitQ hq{ c->frame.dHits.as<float>(), NQ };
    {
        // 16-byte hit records where they are possible: the world-only triangle kernels (every mesh hit names its shading record) and an instance
        // count and a record count that share 32 bits with the all-ones word left for a miss
        const bool worldKernels = trace_build(c, false) >= TB_WORLD;
        const uint32_t range = std::max(1u, c->accel.hitPrimRange); // shading records (or mesh-local indices), light proxies' triangles, curve segments: skh_build_accel
        uint32_t B = 1;
        while (B < 31u && (1u << B) < range)
            ++B;
        hq.primBits = (c->opt.compactHits && worldKernels && c->accel.nShadeRecords != 0u && (uint64_t)c->scene.nInstances <= (1ull << (32u - B)) - 1ull && (1ull << B) >= range) ? B : 0u;
        hq.direct = c->accel.directRecords;
        hq.recClamp = c->accel.nShadeRecords ? c->accel.nShadeRecords - 1u : 0u;
    }
    rp.hq = hq;
    fill_queue_constants(c, rp);
    // dCounts: 260 queues (2 per bounce) x SKH_SHARDS queue-length words, then the ray-fetch cursors (8 per trace launch); every word
    // that is the target of atomics has a 128-byte line of its own (returning atomics on one line serialise at ~88 per microsecond)
    uint32_t* counts = rp.counts = c->frame.dCounts.as<uint32_t>();
    const uint32_t QW = rp.QW = SKH_COUNT_STRIDE * SKH_SHARDS; // words per queue's lengths
    rp.fetch = counts + QW * 2 * SKH_MAX_LAUNCH_ROUNDS;
    // shadow[b] on a second stream: it depends on shade[b] only, and so does closest[b+1]; each fills the other's tail.  Ray
    // sorting shares scratch buffers between the two and keeps everything on one stream.
    // overlap 1 (default): passes up to 32 M paths -- a rank's share of an N-GPU frame, the one-sub-frame-per-call pattern and its
    // speculative passes.  Up to 8 M paths both kernels run on reduced grids (16 + 16 waves per CU: +7 % at 2 M paths); above that on
    // full grids, where the second kernel's blocks simply take the slots the first one's finishing waves leave (1/8 share of a 1080p
    // frame: 24.26 -> 23.87 ms, 93.3 -> 94.9 % of 1/8 of the full frame; 1/4: 97.0 -> 97.8 %).  The full single-GPU frame (64 M paths
    // per pass) gains 0.5 % and stays on one stream so that its per-kernel hipEvent spans do not overlap.  overlap 2: always, reduced grids.
    rp.smallPass = NP <= (1u << 23) || c->opt.overlap == 2;
    rp.useOverlap = (c->opt.overlap == 2 || (c->opt.overlap == 1 && NP <= (1u << 25))) && fp.debug != 1;
    const uint32_t rounds = rp.rounds = fp.maxDepth;
    // Cutouts (skh_set_material_cutouts), only in a context where one is in use: k_cutout and its continuation rounds between a bounce's closest-hit launch and k_shade, and
    // a closest-hit launch with the same rounds behind it in the any-hit launch's place.  Per bounce and side cutout_rounds x SKH_CUT_WORDS words, behind the fetch cursors.
    const bool cutOn = rp.cutOn = cut_stage_on(c);
    rp.cutBounceWords = 2u * c->opt.cutoutRounds * SKH_CUT_WORDS;
    rp.cutWords = rp.fetch + 16 * SKH_FETCH_STRIDE * (rounds + 1);
    rp.cutQ[0] = queue(c->cut.dQ[0]), rp.cutQ[1] = queue(c->cut.dQ[1]), rp.cutSQ[0] = queue(c->cut.dShadowQ[0]), rp.cutSQ[1] = queue(c->cut.dShadowQ[1]);
    rp.cutH = rp.cutSH0 = rp.cutSH1 = hq; // (records as the closest-hit launches of this pass write them)
    rp.cutH.base = c->cut.dHits.as<float>(), rp.cutSH0.base = c->cut.dShadowHits[0].as<float>(), rp.cutSH1.base = c->cut.dShadowHits[1].as<float>();
    // fractional opacity (skh_set_material_blend), where it is in use: what the draw's path identity needs of the frame, and the contribution records, writable
    rp.blp = make_blend(c);
    rp.blp.tileXY = rp.tiles, rp.blp.sppTotal = fp.sppTotal, rp.blp.numSlots = fp.numSlots, rp.blp.tileShift = fp.tileShift;
    rp.blp.contrib = c->frame.dContrib.as<float4>();
    rp.split = c->opt.tailSplit < 0 && rp.smallPass && NP >= (1u << 17);
    // One sub-frame of one sample, accumulated in this call (the reference caller's pattern): its sums ARE the path's radiance and event word -- the batch kernel reads
    // them where they lie (0.0f + radiance, / 1.0f: the same operations), and the k_collect launch and its 11 planes of sums are not needed.
    const bool oneSampleDirect = batch == 1 && fp.samplesThisLaunch == 1 && plan.finalize && fp.finalFirst == 0 && fp.finalCount == 1;
    for (uint32_t s = 0; plan.trace && s < fp.samplesThisLaunch; ++s)
    {
        // (a cutout in use: the words of its continuation rounds lie behind the fetch cursors this sample uses -- one memset for all of them)
        SKH_TRY(c, hipMemsetAsync(counts, 0, sizeof(uint32_t) * (QW * 2 * SKH_MAX_LAUNCH_ROUNDS + 16 * SKH_FETCH_STRIDE * (rounds + 1) + (size_t)(cutOn ? rounds : 0u) * rp.cutBounceWords), st));
        rp.blp.sampleBase = fp.subframeIndex + s;
        {
            SpanGuard g(c, KC_RAYGEN);
            const uint32_t launchCells = (c->frame.raygenBlocksPerSub + order.launchCell - 1u) / order.launchCell;
            k_raygen<<<launchCells * order.launchCell * fp.batch, 512, 0, st>>>(fp, rp.tiles, s, rp.rq[0], counts, rp.ps, order.qBase, order.subStride, c->frame.raygenBlocksPerSub, raygenValid,
                                                                                 order.launchCell, order.perWave);
        }
        for (uint32_t b = 0; b < rounds; ++b)
        {
            render_bounce(c, rp, s, b);
            if (fp.debug == 1)
                break;
        }
        if (rp.useOverlap)
            (void)hipStreamWaitEvent(st, c->dev.evShadow, 0);
        {
            SpanGuard g(c, KC_ACCUM);
            k_add_stats<<<1, 64, 0, st>>>(counts, rounds, c->timing.dStats.as<StatsDev>());
            if (batch == 1 && !oneSampleDirect)
                k_collect<<<(c->frame.numSlots + 255) / 256, 256, 0, st>>>(fp, rp.tiles, s, rp.ps, c->frame.dSums.as<float>());
        }
    }
    render_accumulate(c, rp, plan, oneSampleDirect, d_image);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        c->dev.err = std::string("render launch: ") + hipGetErrorString(e);
        return SKH_FAIL;
    }
    return SKH_OK;
}

skh_status skh_render_subframes(skh_context* c, const skh_frame_params* params, uint32_t n_subframes, void* d_image)
{
    if (!c || !params)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (c->frame.width == 0)
    {
        c->dev.err = "skh_render_subframe: call skh_resize first";
        return SKH_INVALID_ARGUMENT;
    }
    skh_status s = ensure_ready(c);
    if (s != SKH_OK)
        return s;
    if (n_subframes != 1)
        spec_drop(c, false, true); // (the path state is about to be reused)
    else
        spec_drop(c, true);
    skh_frame_params p = *params;
    // single-sample sub-frames are traced `batchCapacity` at a time when that gives the GPU more rays per launch
    const uint32_t cap = (p.samples_this_launch == 1 && p.debug != 1) ? c->frame.batchCapacity : 1u;
    const bool adaptive = adapt_applies(c, p) && n_subframes != 0u;
    if (adaptive && (s = adapt_prepare(c, p)) != SKH_OK)
        return s;
    for (uint32_t k = 0; k < n_subframes;)
    {
        if (adaptive && c->adapt.activeTiles == 0u)
        {
            // every tile is frozen: the rest of the call traces nothing
            c->adapt.pixelObsSaved += (uint64_t)c->frame.raygenValidPerSub * (n_subframes - k);
            break;
        }
        uint32_t b = std::min(cap, n_subframes - k);
        if (adaptive)
            b = std::min(b, adapt_to_next_check(c)); // (a batch never straddles a check)
        RenderPlan plan;
        plan.batch = b, plan.adaptive = adaptive;
        s = render_one(c, &p, plan, d_image);
        if (s != SKH_OK || (adaptive && (s = adapt_after_pass(c, p, b)) != SKH_OK))
            return s;
        p.subframe_index += p.samples_this_launch * b;
        k += b;
    }
    if (adaptive)
        adapt_fill(c, p, d_image);
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream)); // the reference's render() is synchronous (OptixRender.cpp:1012)
    if (c->opt.timing)
        harvest_spans(c);
    return check_stack_overflow(c, "skh_render_subframes");
}

// true when b continues the frame a belongs to: everything equal except the sub-frame index, which advances by `step`
static bool same_frame(const skh_frame_params& a, const skh_frame_params& b, uint32_t step)
{
    skh_frame_params x = a, y = b;
    if (y.subframe_index != x.subframe_index + step)
        return false;
    x.subframe_index = y.subframe_index = 0;
    return memcmp(&x, &y, sizeof(x)) == 0;
}

// speculate_async: start tracing the pass that follows the one being consumed.  Nothing is in flight and c->dev.stream is idle here.
static skh_status spec_launch_next(skh_context* c)
{
    skh_context::Speculation& sp = c->spec;
    if (!c->opt.speculateAsync || !sp.valid || sp.nextInFlight || c->opt.timing)
        return SKH_OK; // (per-kernel hipEvent spans are harvested at every call: timing runs keep the synchronous scheme)
    const uint32_t nextStart = sp.params.subframe_index + sp.count;
    if (nextStart >= sp.params.spp_total)
        return SKH_OK;
    const uint32_t cap = std::min(c->opt.speculateMax, c->frame.batchCapacity);
    const uint32_t n = std::min(std::min(std::max(2u, sp.count * c->opt.speculateGrow), cap), sp.params.spp_total - nextStart);
    const uint32_t other = sp.buf ^ 1u;
    if (other == 1u)
    {
        const uint32_t stride = c->frame.numSlots * cap;
        skh_status s = dev_alloc(c, c->spec.dPathB, sizeof(float) * SKH_PATH_FLOATS * (size_t)stride);
        if (s != SKH_OK)
            return s;
        c->spec.pathBStride = stride;
    }
    SKH_TRY(c, hipMemcpy(sp.statsMark, c->timing.dStats.p, sizeof(sp.statsMark), hipMemcpyDeviceToHost));
    sp.nextParams = sp.params;
    sp.nextParams.subframe_index = nextStart;
    sp.nextCount = n;
    RenderPlan plan; // trace only, into the other path-state buffer
    plan.batch = n, plan.finalCount = 0, plan.pathSel = other, plan.finalize = false;
    skh_status s = render_one(c, &sp.nextParams, plan, nullptr);
    if (s != SKH_OK)
        return s;
    sp.nextInFlight = true;
    return SKH_OK;
}

skh_status skh_render_subframe(skh_context* c, const skh_frame_params* params, void* d_image)
{
    if (!c || !params)
        return SKH_INVALID_ARGUMENT;
    skh_context::Speculation& sp = c->spec;
    const bool eligible = c->opt.speculateMax > 1 && params->samples_this_launch == 1 && params->debug == 0 && c->frame.width != 0 && c->frame.batchCapacity > 1 &&
                          !c->adapt.on; // (an adaptive context traces nothing ahead: a pass that begins at a check cannot start before the check has run)
    if (!eligible)
    {
        spec_drop(c, false, true);
        return skh_render_subframes(c, params, 1, d_image);
    }
    (void)hipSetDevice(c->dev.device);
    skh_status s;
    if (sp.nextInFlight && sp.valid && sp.consumed >= sp.count && same_frame(sp.nextParams, *params, 0))
    {
        // the caller has collected the whole pass and continues into the one in flight: wait for it, make it the current pass
        unsigned long long after[2] = { 0, 0 };
        SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
        SKH_TRY(c, hipMemcpy(after, c->timing.dStats.p, sizeof(after), hipMemcpyDeviceToHost));
        sp.nextInFlight = false;
        sp.passRadiance = after[0] - sp.statsMark[0];
        sp.passShadow = after[1] - sp.statsMark[1];
        sp.buf ^= 1u;
        sp.params = sp.nextParams;
        sp.count = sp.nextCount;
        sp.consumed = 0;
        sp.lastBatch = sp.nextCount;
        if ((s = check_stack_overflow(c, "skh_render_subframe")) != SKH_OK)
            return s;
    }
    if (sp.valid && sp.consumed < sp.count && same_frame(sp.params, *params, sp.consumed))
    {
        // this sub-frame was traced ahead: its radiances wait in the path state, only its accumulation step is left (beside a pass in
        // flight it runs on its own stream)
        hipStream_t fin = side_stream(c);
        RenderPlan plan; // the accumulation step of sub-frame sp.consumed of the pass
        plan.batch = sp.count, plan.trace = false, plan.finalFirst = sp.consumed, plan.finalCount = 1, plan.pathSel = sp.buf, plan.finStream = fin;
        if ((s = render_one(c, &sp.params, plan, d_image)) != SKH_OK)
            return s;
        sp.consumed++;
        sp.last = *params;
        sp.haveLast = true;
        sp.streak++;
        SKH_TRY(c, hipStreamSynchronize(fin));
        if (c->opt.timing && !sp.nextInFlight)
            harvest_spans(c);
        if (sp.consumed == 1)
            return spec_launch_next(c); // (first delivery of a pass that was itself traced in flight)
        return SKH_OK;
    }
    // a fresh pass.  How far ahead: nothing on the first call of a frame or after any change (interactive camera motion restarts at
    // sub-frame 0 every call and must not pay for samples it will throw away); doubling while the caller keeps continuing the frame
    const bool continues = sp.haveLast && same_frame(sp.last, *params, 1);
    sp.streak = continues ? sp.streak + 1 : 0;
    uint32_t ahead = 1;
    if (continues && params->spp_total > params->subframe_index)
        ahead = std::min(std::min(std::max(2u, sp.lastBatch * c->opt.speculateGrow), std::min(c->opt.speculateMax, c->frame.batchCapacity)), params->spp_total - params->subframe_index);
    spec_drop(c, true);
    if ((s = ensure_ready(c)) != SKH_OK)
        return s;
    if (ahead <= 1)
    {
        sp.lastBatch = 1;
        sp.last = *params;
        sp.haveLast = true;
        return skh_render_subframes(c, params, 1, d_image);
    }
    unsigned long long before[2] = { 0, 0 }, after[2] = { 0, 0 }; // (StatsDev starts with raysRadiance, raysShadow; the stream is idle here)
    SKH_TRY(c, hipMemcpy(before, c->timing.dStats.p, sizeof(before), hipMemcpyDeviceToHost));
    RenderPlan plan; // `ahead` sub-frames traced, the first one delivered
    plan.batch = ahead, plan.finalCount = 1;
    if ((s = render_one(c, params, plan, d_image)) != SKH_OK)
        return s;
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    SKH_TRY(c, hipMemcpy(after, c->timing.dStats.p, sizeof(after), hipMemcpyDeviceToHost));
    sp.passRadiance = after[0] - before[0];
    sp.passShadow = after[1] - before[1];
    sp.valid = true;
    sp.buf = 0;
    sp.params = *params;
    sp.count = ahead;
    sp.consumed = 1;
    sp.lastBatch = ahead;
    sp.last = *params;
    sp.haveLast = true;
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    if (c->opt.timing)
        harvest_spans(c);
    if ((s = check_stack_overflow(c, "skh_render_subframe")) != SKH_OK)
        return s;
    return spec_launch_next(c);
}

skh_status skh_tonemap(skh_context* c, void* d_image, uint32_t width, uint32_t height, uint32_t type, const float exposure[3], float gamma)
{
    if (!c || !d_image || !exposure)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    const uint32_t n = width * height; // the reference's kernels test `> n` (Tonemappers.cu:20); this build uses >= n
    hipStream_t st = side_stream(c); // (beside a pass traced ahead: not behind it)
    k_tonemap<<<(n + 255) / 256, 256, 0, st>>>(reinterpret_cast<float4*>(d_image), n, type, exposure[0], exposure[1], exposure[2], gamma);
    SKH_TRY(c, hipStreamSynchronize(st));
    return SKH_OK;
}

skh_status skh_buffer_alloc(skh_context* c, size_t bytes, void** out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    *out = nullptr;
    SKH_TRY(c, hipMalloc(out, bytes ? bytes : 16));
    // (cleared on the stream that skh_buffer_upload and the image passes use, and waited for: a null-stream memset queues behind a pass traced ahead on the main
    // stream and would land after an upload or a kernel that the side stream has already run on the new buffer)
    hipStream_t st = side_stream(c);
    SKH_TRY(c, hipMemsetAsync(*out, 0, bytes ? bytes : 16, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    return SKH_OK;
}
skh_status skh_buffer_free(skh_context* c, void* p)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (p)
        SKH_TRY(c, hipFree(p));
    return SKH_OK;
}
skh_status skh_buffer_download(skh_context* c, const void* d, void* host, size_t bytes)
{
    if (!c || !d || !host)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (c->spec.nextInFlight)
    {
        // (the image was written by an accumulation step on stream3, which has completed; c->dev.stream is busy with the pass traced
        // ahead and a null-stream copy would wait for it)
        SKH_TRY(c, hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, c->dev.stream3));
        SKH_TRY(c, hipStreamSynchronize(c->dev.stream3));
        return SKH_OK;
    }
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    SKH_TRY(c, hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost));
    return SKH_OK;
}
// (the same choice of stream: beside a pass traced ahead, else behind whatever c->dev.stream still does with the buffer)
skh_status skh_buffer_upload(skh_context* c, void* d, const void* host, size_t bytes)
{
    if (!c || !d || !host)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    hipStream_t st = side_stream(c);
    SKH_TRY(c, hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st));
    SKH_TRY(c, hipStreamSynchronize(st));
    return SKH_OK;
}

skh_status skh_host_register(skh_context* c, void* host, size_t bytes)
{
    if (!c || !host || !bytes)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    SKH_TRY(c, hipHostRegister(host, bytes, hipHostRegisterDefault));
    return SKH_OK;
}
skh_status skh_host_unregister(skh_context* c, void* host)
{
    if (!c || !host)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    SKH_TRY(c, hipHostUnregister(host));
    return SKH_OK;
}

static skh_status detile_to(skh_context* c, const DevBuf& src, void* d_dst)
{
    k_detile<<<(c->frame.numSlots + 255) / 256, 256, 0, c->dev.stream>>>(src.as<float4>(), c->frame.dTileXY.as<uint32_t>(), c->frame.numSlots, c->frame.tileShift,
                                                              c->frame.width, c->frame.height, reinterpret_cast<float4*>(d_dst));
    return SKH_OK;
}

static skh_status read_slots(skh_context* c, const DevBuf& src, float* host)
{
    if (!c || !host || !c->frame.width)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    const size_t bytes = sizeof(float4) * (size_t)c->frame.width * c->frame.height;
    skh_status s = dev_alloc(c, c->frame.dScratchImage, bytes);
    if (s != SKH_OK)
        return s;
    SKH_TRY(c, hipMemsetAsync(c->frame.dScratchImage.p, 0, bytes, c->dev.stream));
    detile_to(c, src, c->frame.dScratchImage.p);
    SKH_TRY(c, hipMemcpyAsync(host, c->frame.dScratchImage.p, bytes, hipMemcpyDeviceToHost, c->dev.stream));
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}
skh_status skh_read_accum(skh_context* c, float* host_rgba)
{
    return read_slots(c, c->frame.dAccum, host_rgba);
}
skh_status skh_read_adaptive(skh_context* c, float* host_rgba)
{
    if (!c || !host_rgba || !c->frame.width)
        return SKH_INVALID_ARGUMENT;
    if (!c->adapt.on || !c->adapt.ready)
    {
        memset(host_rgba, 0, sizeof(float) * 4 * (size_t)c->frame.width * c->frame.height); // (no frame has begun: nothing observed)
        return SKH_OK;
    }
    return read_slots(c, c->adapt.dState, host_rgba);
}
skh_status skh_read_aov(skh_context* c, uint32_t which, float* host_rgba)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    return read_slots(c, which == 0 ? c->frame.dDiffuse : c->frame.dSpecular, host_rgba);
}
skh_status skh_copy_accum(skh_context* c, void* d_dst)
{
    if (!c || !d_dst)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    detile_to(c, c->frame.dAccum, d_dst);
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}
// the diffuse / specular AOV accumulators to a device image: what render() hands back once all samples are done and the debug view
// is 2 / 3 (OptixRender.cpp:1029-1042: cudaMemcpy(params.image, params.diffuse | params.specular))
skh_status skh_copy_aov(skh_context* c, uint32_t which, void* d_dst)
{
    if (!c || !d_dst || which > 1u)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (c->frame.width == 0)
    {
        c->dev.err = "skh_copy_aov: call skh_resize first";
        return SKH_INVALID_ARGUMENT;
    }
    detile_to(c, which == 0 ? c->frame.dDiffuse : c->frame.dSpecular, d_dst);
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}
skh_status skh_copy_accum_tiles(skh_context* c, void* d_dst)
{
    if (!c || !d_dst)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    SKH_TRY(c, hipMemcpyAsync(d_dst, c->frame.dAccum.p, sizeof(float4) * (size_t)c->frame.numSlots, hipMemcpyDeviceToDevice, c->dev.stream));
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}
skh_status skh_scatter_tiles(skh_context* c, const void* d_src_tiles, const uint32_t* tile_xy, uint32_t n_tiles, uint32_t tile_size,
                             void* d_dst, uint32_t width, uint32_t height)
{
    if (!c || !d_src_tiles || !tile_xy || !d_dst || (tile_size & (tile_size - 1)))
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    // (tile list kept in a context buffer: no allocation per call; tiles whose origin lies outside the image -- the padding
    // of a gathered multi-rank tile set -- write nothing)
    skh_status s = dev_upload(c, c->multi.dScatterXY, tile_xy, sizeof(uint32_t) * 2 * (size_t)n_tiles);
    if (s != SKH_OK)
        return s;
    uint32_t shift = 0;
    while ((1u << shift) < tile_size)
        ++shift;
    const uint32_t slots = n_tiles * tile_size * tile_size;
    k_detile<<<(slots + 255) / 256, 256, 0, c->dev.stream>>>(reinterpret_cast<const float4*>(d_src_tiles), c->multi.dScatterXY.as<uint32_t>(), slots, shift,
                                                        width, height, reinterpret_cast<float4*>(d_dst));
    hipError_t e = hipStreamSynchronize(c->dev.stream);
    if (e != hipSuccess)
    {
        c->dev.err = std::string("skh_scatter_tiles: ") + hipGetErrorString(e);
        return SKH_FAIL;
    }
    return SKH_OK;
}

// ---- multi-GPU tile gather (RCCL, loaded on first use) ----
namespace
{
struct RcclApi
{
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr; // optional
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr; // optional
    std::string why;
    bool overridden = false; // bound to SKH_RCCL_LIB instead of librccl (tests)
};
static bool rccl_load(RcclApi& api);
RcclApi* rccl()
{
    // (contexts on different GPUs may be driven from different threads: load once)
    static RcclApi api;
    static std::once_flag once;
    static bool ok = false;
    std::call_once(once, [] { ok = rccl_load(api); });
    return ok ? &api : nullptr;
}
static bool rccl_load(RcclApi& api)
{
    // SKH_RCCL_LIB (tests only): the library to bind instead -- tests/cpp/rccl_double.cpp, a stand-in for N ranks SHARING one GPU, so that the
    // N > 1 branch of skh_gather_tiles runs on a 1-GPU box.  RTLD_LOCAL: its nccl* symbols must not shadow the real ones PyTorch has loaded.
    if (const char* over = getenv("SKH_RCCL_LIB"))
    {
        if (!(api.lib = dlopen(over, RTLD_NOW | RTLD_LOCAL)))
        {
            api.why = std::string("SKH_RCCL_LIB=") + over + ": " + dlerror();
            return false;
        }
        api.overridden = true;
    }
    // (a process that uses PyTorch has its librccl.so.1 loaded already: the same soname resolves to that copy)
    for (const char* name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" })
        if (api.lib || (api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL)))
            break;
    if (!api.lib)
    {
        api.why = "librccl.so.1 not found";
        return false;
    }
#define SKH_SYM(field, sym) (*(void**)(&api.field) = dlsym(api.lib, sym))
    SKH_SYM(GetUniqueId, "ncclGetUniqueId");
    SKH_SYM(CommInitRank, "ncclCommInitRank");
    SKH_SYM(CommDestroy, "ncclCommDestroy");
    SKH_SYM(Send, "ncclSend");
    SKH_SYM(Recv, "ncclRecv");
    SKH_SYM(GroupStart, "ncclGroupStart");
    SKH_SYM(GroupEnd, "ncclGroupEnd");
    SKH_SYM(GetErrorString, "ncclGetErrorString");
    SKH_SYM(CommCount, "ncclCommCount");
    SKH_SYM(CommUserRank, "ncclCommUserRank");
#undef SKH_SYM
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.Send || !api.Recv || !api.GroupStart || !api.GroupEnd)
    {
        api.why = "librccl.so.1 lacks the point-to-point API";
        api.lib = nullptr;
        return false;
    }
    return true;
}
} // namespace

skh_status skh_comm_unique_id(void* out_id)
{
    static_assert(sizeof(ncclUniqueId) == SKH_COMM_ID_BYTES, "id size");
    RcclApi* r = rccl();
    if (!out_id || !r)
        return out_id ? SKH_FAIL : SKH_INVALID_ARGUMENT;
    ncclUniqueId id;
    if (r->GetUniqueId(&id) != ncclSuccess)
        return SKH_FAIL;
    memcpy(out_id, &id, sizeof(id));
    return SKH_OK;
}

skh_status skh_comm_init(skh_context* c, const void* id, int world_size, int rank)
{
    if (!c || !id || world_size < 1 || rank < 0 || rank >= world_size)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    RcclApi* r = rccl();
    if (!r)
    {
        c->dev.err = "skh_comm_init: RCCL is not available (librccl.so.1)";
        return SKH_FAIL;
    }
    if (c->multi.comm)
        (void)skh_comm_destroy(c);
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    const ncclResult_t e = r->CommInitRank(&c->multi.comm, world_size, uid, rank);
    if (e != ncclSuccess)
    {
        c->multi.comm = nullptr;
        c->dev.err = std::string("skh_comm_init: ncclCommInitRank: ") + (r->GetErrorString ? r->GetErrorString(e) : "error");
        return SKH_FAIL;
    }
    c->multi.world = world_size;
    c->multi.rank = rank;
    return SKH_OK;
}

skh_status skh_comm_info(skh_context* c, int* out_world, int* out_rank, int* out_rccl_ranks)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    if (out_world)
        *out_world = c->multi.world;
    if (out_rank)
        *out_rank = c->multi.rank;
    if (out_rccl_ranks)
    {
        // what RCCL itself says about the communicator (ncclCommCount): 0 = no communicator (world size 1, or the caller gathers another way)
        int n = 0;
        RcclApi* r = c->multi.comm ? rccl() : nullptr;
        if (r && r->CommCount && r->CommCount(c->multi.comm, &n) != ncclSuccess)
            n = -1;
        *out_rccl_ranks = n;
    }
    return SKH_OK;
}

skh_status skh_comm_destroy(skh_context* c)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (c->multi.comm)
    {
        (void)hipStreamSynchronize(c->dev.stream);
        RcclApi* r = rccl();
        if (r)
            (void)r->CommDestroy(c->multi.comm);
        c->multi.comm = nullptr;
    }
    c->multi.world = 1;
    c->multi.rank = 0;
    return SKH_OK;
}

skh_status skh_gather_tiles(skh_context* c, uint32_t max_tiles, void* d_recv, int root)
{
    if (!c || root < 0 || root >= c->multi.world || max_tiles < c->frame.numTiles || (c->multi.rank == root && !d_recv))
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (c->multi.world > 1 && !c->multi.comm)
    {
        c->dev.err = "skh_gather_tiles: call skh_comm_init first";
        return SKH_INVALID_ARGUMENT;
    }
    const size_t tilePixels = (size_t)c->frame.tileSize * c->frame.tileSize;
    const size_t chunk = (size_t)max_tiles * tilePixels; // float4 per rank
    const size_t mine = (size_t)c->frame.numTiles * tilePixels;
    const bool isRoot = c->multi.rank == root;
    // the root's own share goes straight into its slot of the receive buffer; a sender stages its tiles (zero-padded) once
    float4* dst = isRoot ? reinterpret_cast<float4*>(d_recv) + (size_t)root * chunk : nullptr;
    if (!isRoot)
    {
        skh_status s = dev_alloc(c, c->multi.dTileSend, sizeof(float4) * chunk);
        if (s != SKH_OK)
            return s;
        dst = c->multi.dTileSend.as<float4>();
    }
    SKH_TRY(c, hipMemcpyAsync(dst, c->frame.dAccum.p, sizeof(float4) * mine, hipMemcpyDeviceToDevice, c->dev.stream));
    if (chunk > mine)
        SKH_TRY(c, hipMemsetAsync(dst + mine, 0, sizeof(float4) * (chunk - mine), c->dev.stream));
    if (c->multi.world > 1)
    {
        RcclApi* r = rccl();
        ncclResult_t e = r->GroupStart();
        if (isRoot)
        {
            for (int k = 0; k < c->multi.world && e == ncclSuccess; ++k)
                if (k != root)
                    e = r->Recv(reinterpret_cast<float4*>(d_recv) + (size_t)k * chunk, chunk * 4, ncclFloat, k, c->multi.comm, c->dev.stream);
        }
        else if (e == ncclSuccess)
            e = r->Send(dst, chunk * 4, ncclFloat, root, c->multi.comm, c->dev.stream);
        const ncclResult_t e2 = r->GroupEnd();
        if (e != ncclSuccess || e2 != ncclSuccess)
        {
            c->dev.err = std::string("skh_gather_tiles: ") + (r->GetErrorString ? r->GetErrorString(e != ncclSuccess ? e : e2) : "RCCL error");
            return SKH_FAIL;
        }
    }
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}

// ---- raw ray queries ----
// raw queries: ray k of the caller sits in shard k / per at offset k % per (per = rays per shard, a multiple of 64)
__global__ void k_rays_aos_to_soa(const skh_ray* __restrict__ rays, uint32_t n, uint32_t per, RayQ rq)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const skh_ray r = rays[k];
    const uint32_t g = k / per, i = g * rq.region + (k - g * per);
    rq.plane(0)[i] = r.origin[0];
    rq.plane(1)[i] = r.origin[1];
    rq.plane(2)[i] = r.origin[2];
    rq.plane(3)[i] = r.dir[0];
    rq.plane(4)[i] = r.dir[1];
    rq.plane(5)[i] = r.dir[2];
    rq.plane(6)[i] = r.tmin;
    rq.plane(7)[i] = r.tmax;
    rq.ids()[i] = k;
}
__global__ void k_hits_soa_to_aos(HitQ hq, uint32_t n, uint32_t per, uint32_t region, uint32_t mode, skh_hit* __restrict__ hits,
                                  const skh_instance* __restrict__ shadeInst /* light_id of a mesh instance = its first shading record */)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t g = k / per, i = g * region + (k - g * per);
    skh_hit h;
    if (mode == SKH_TRACE_SHADOW)
    {
        h.t = hq.base[i];
        h.instance_id = h.prim_id = 0xffffffffu;
        h.u = h.v = 0.0f;
    }
    else
    {
        const float4 r0 = hq.rec(i)[0], r1 = hq.rec(i)[1];
        h.t = r0.x, h.u = r0.y, h.v = r0.z;
        h.instance_id = __float_as_uint(r1.x);
        h.prim_id = __float_as_uint(r1.y);
        // a hit on a baked triangle carries the index of its shading record (k_gather_tris): back to the primitive index inside the mesh
        if (h.instance_id != 0xffffffffu && (h.prim_id & SKH_PRIM_DIRECT))
            h.prim_id = (h.prim_id & ~SKH_PRIM_DIRECT) - shadeInst[h.instance_id].light_id;
    }
    hits[k] = h;
}

#include "skh_probes.inc"

// skh_trace_device's path: `cls` is the kernel class its spans are counted under (skh_render_aovs traces through here under a class of its own)
static skh_status trace_device_as(skh_context* c, const void* d_rays, uint32_t n_rays, uint32_t mode, void* d_hits, uint32_t repeat, KernelClass cls)
{
    if (!c || (n_rays && (!d_rays || !d_hits)) || mode > 1)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    skh_status s = ensure_ready(c);
    if (s != SKH_OK || n_rays == 0)
        return s;
    // a speculative pass in flight shares the stack-overflow flag and the overflow area with this query: wait for it and drop it first, so
    // that an overflow is attributed to the call that caused it
    spec_drop(c, true);
    DevBuf q, h, cnt;
    const uint32_t per = (((n_rays + SKH_SHARDS - 1u) / SKH_SHARDS) + 63u) & ~63u; // rays per shard = the shard's region
    const size_t NQ = (size_t)SKH_SHARDS * per;
    SKH_CHECK(dev_alloc(c, q, sizeof(float) * 9 * NQ));
    SKH_CHECK(dev_alloc(c, h, sizeof(float) * 8 * NQ));
    // a cutout in use (skh_set_material_cutouts): the continuation rounds run on the internal records, before k_hits_soa_to_aos; their words lie behind the fetch cursors
    const bool cutOn = cut_stage_on(c);
    const size_t cutWordCount = cutOn ? (size_t)c->opt.cutoutRounds * SKH_CUT_WORDS : 0u;
    DevBuf cq0, cq1, h2, h0;
    SKH_CHECK(dev_alloc(c, cnt, sizeof(uint32_t) * (SKH_SHARDS * SKH_COUNT_STRIDE + 8 * SKH_FETCH_STRIDE + cutWordCount)));
    if (cutOn)
    {
        SKH_CHECK(dev_alloc(c, cq0, sizeof(float) * 9 * NQ));
        SKH_CHECK(dev_alloc(c, cq1, sizeof(float) * 9 * NQ));
        SKH_CHECK(dev_alloc(c, h2, sizeof(float) * 8 * NQ));
        if (mode == SKH_TRACE_SHADOW)
            SKH_CHECK(dev_alloc(c, h0, sizeof(float) * 8 * NQ));
    }
    if (!c->frame.traceBlocks)
        c->frame.traceBlocks = (uint32_t)c->dev.numCUs * c->opt.wavesPerCU;
    SKH_CHECK(dev_alloc(c, c->frame.dOvf, sizeof(int) * (size_t)(SKH_STACK_OVF + SKH_TAIL_EXTRA) * (uint32_t)c->dev.numCUs * std::max(std::max(c->opt.wavesPerCU, c->opt.wavesPerCUWorld), std::max(c->opt.wavesPerCUShadow, c->opt.wavesPerCUShadowWorld)) * SKH_TRACE_BLOCK));
    RayQ rq{ q.as<float>(), (uint32_t)NQ, per };
    HitQ hq{ h.as<float>(), (uint32_t)NQ };
    PathS ps{ nullptr, 0 };
    uint32_t* dcount = cnt.as<uint32_t>();
    uint32_t* dfetch = dcount + SKH_SHARDS * SKH_COUNT_STRIDE;
    uint32_t hcount[SKH_SHARDS * SKH_COUNT_STRIDE] = { 0 };
    for (uint32_t g = 0; g < SKH_SHARDS; ++g)
        hcount[g * SKH_COUNT_STRIDE] = std::min(per, n_rays - std::min(n_rays, g * per));
    SKH_TRY(c, hipMemcpyAsync(dcount, hcount, sizeof(hcount), hipMemcpyHostToDevice, c->dev.stream));
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream)); // (hcount lives on this stack frame)
    const DevScene sc = make_dev_scene(c);
    k_rays_aos_to_soa<<<(n_rays + 255) / 256, 256, 0, c->dev.stream>>>(reinterpret_cast<const skh_ray*>(d_rays), n_rays, per, rq);
    for (uint32_t r = 0; r < std::max(1u, repeat); ++r)
    {
        (void)hipMemsetAsync(dfetch, 0, sizeof(uint32_t) * (8 * SKH_FETCH_STRIDE + cutWordCount), c->dev.stream);
        SpanGuard g(c, cls);
        const bool shadow = mode == SKH_TRACE_SHADOW;
        const TraceLaunch t{ rq, dcount, dfetch, hq, ps, nullptr, c->dev.stream, shadow, 0u, false };
        // (a cutout in use) no sample: a blend hit counts iff a > 0; a shadow query's result is one float per ray
        CutRounds cr{ { RayQ{ cq0.as<float>(), (uint32_t)NQ, per }, RayQ{ cq1.as<float>(), (uint32_t)NQ, per } }, HitQ{ h0.as<float>(), (uint32_t)NQ }, HitQ{ h2.as<float>(), (uint32_t)NQ },
                      shadow ? hq.base : nullptr, dfetch + 8 * SKH_FETCH_STRIDE, n_rays, make_blend(c) };
        cr.bl.raw = 1u;
        trace_step(c, sc, t, shadow, cutOn ? &cr : nullptr);
    }
    k_hits_soa_to_aos<<<(n_rays + 255) / 256, 256, 0, c->dev.stream>>>(hq, n_rays, per, per, mode, reinterpret_cast<skh_hit*>(d_hits), c->accel.dShadeInst.as<skh_instance>());
    hipError_t e = hipStreamSynchronize(c->dev.stream);
    if (e != hipSuccess || (e = hipGetLastError()) != hipSuccess)
    {
        c->dev.err = std::string("skh_trace: ") + hipGetErrorString(e);
        return SKH_FAIL;
    }
    if (c->opt.timing)
        harvest_spans(c);
    return check_stack_overflow(c, "skh_trace");
}

skh_status skh_trace_device(skh_context* c, const void* d_rays, uint32_t n_rays, uint32_t mode, void* d_hits, uint32_t repeat)
{
    return trace_device_as(c, d_rays, n_rays, mode, d_hits, repeat, mode == SKH_TRACE_SHADOW ? KC_TRACE_SHADOW : KC_TRACE_CLOSEST);
}

skh_status skh_trace(skh_context* c, const skh_ray* rays, uint32_t n_rays, uint32_t mode, skh_hit* hits)
{
    if (!c || (n_rays && (!rays || !hits)))
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (n_rays == 0)
        return SKH_OK;
    DevBuf dr, dh;
    SKH_CHECK(dev_upload(c, dr, rays, sizeof(skh_ray) * (size_t)n_rays));
    SKH_CHECK(dev_alloc(c, dh, sizeof(skh_hit) * (size_t)n_rays));
    skh_status s = skh_trace_device(c, dr.p, n_rays, mode, dh.p, 1);
    if (s == SKH_OK)
    {
        hipError_t e = hipMemcpy(hits, dh.p, sizeof(skh_hit) * (size_t)n_rays, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
        {
            c->dev.err = std::string("skh_trace readback: ") + hipGetErrorString(e);
            s = SKH_FAIL;
        }
    }
    return s;
}

#include "skh_image.inc"

// ---- first-hit AOVs (skh_aov.h): skh_aov_check, skh_render_aovs, skh_get_aov_info ----
static_assert(sizeof(skh_aov_params) == 240 && sizeof(skh_aov_info) == 32, "ABI layout");

// why *p is refused for an image_w x image_h image, or nullptr
static const char* aov_refusal(const skh_aov_params* p, uint32_t image_w, uint32_t image_h)
{
    if (!p)
        return "no parameters";
    if (image_w == 0u || image_h == 0u)
        return "the image is empty (call skh_resize first)";
    const bool whole = p->width == 0u && p->height == 0u;
    if (whole ? (p->x0 != 0u || p->y0 != 0u) : (p->width == 0u || p->height == 0u || p->x0 >= image_w || p->y0 >= image_h || p->width > image_w - p->x0 || p->height > image_h - p->y0))
        return "the region leaves the image or has one zero side";
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(p->view_to_world[k]) || !std::isfinite(p->clip_to_view[k]) || !std::isfinite(p->world_to_clip[k]))
            return "a matrix entry that is not finite";
    if (!std::isfinite(p->tmin) || p->tmin < 0.0f)
        return "tmin negative or not finite";
    if (p->sample_index != SKH_AOV_PIXEL_CENTRE && (p->spp_total == 0u || p->sample_index >= p->spp_total))
        return "sample_index outside the sequence of spp_total samples";
    return reserved_refusal(p->reserved);
}

skh_status skh_aov_check(const skh_aov_params* p, uint32_t image_w, uint32_t image_h)
{
    return aov_refusal(p, image_w, image_h) ? SKH_INVALID_ARGUMENT : SKH_OK;
}

skh_status skh_render_aovs(skh_context* c, const skh_aov_params* p, uint32_t planes, void* const d_planes[SKH_AOV_COUNT])
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    const char* why = aov_refusal(p, c->frame.width, c->frame.height);
    if (!why && (planes == 0u || (planes >> SKH_AOV_COUNT) != 0u))
        why = "no plane asked for, or a bit at or above SKH_AOV_COUNT";
    if (!why && !d_planes)
        why = "no plane pointers";
    for (uint32_t k = 0; !why && k < SKH_AOV_COUNT; ++k)
        if (((planes >> k) & 1u) && !d_planes[k])
            why = "a plane asked for without a buffer";
    if (why)
    {
        c->dev.err = std::string("skh_render_aovs: ") + why;
        return SKH_INVALID_ARGUMENT;
    }
    (void)hipSetDevice(c->dev.device);
    const auto t0 = std::chrono::steady_clock::now();
    SKH_CHECK(ensure_ready(c)); // (the scene record below is the built one's)
    AovP ap;
    memcpy(ap.viewToWorld, p->view_to_world, sizeof(ap.viewToWorld));
    memcpy(ap.clipToView, p->clip_to_view, sizeof(ap.clipToView));
    memcpy(ap.worldToClip, p->world_to_clip, sizeof(ap.worldToClip));
    const bool whole = p->width == 0u && p->height == 0u;
    ap.imageW = c->frame.width, ap.imageH = c->frame.height;
    ap.x0 = p->x0, ap.y0 = p->y0, ap.width = whole ? c->frame.width : p->width;
    const uint32_t regionH = whole ? c->frame.height : p->height;
    ap.sampleIndex = p->sample_index, ap.sppTotal = p->spp_total, ap.tmin = p->tmin;
    const uint64_t total = (uint64_t)ap.width * regionH;
    const uint32_t band = (uint32_t)std::min<uint64_t>(total, c->opt.aovBand);
    DevBuf rays, hits; // (of one band; gone when the call returns)
    SKH_CHECK(dev_alloc(c, rays, sizeof(skh_ray) * (size_t)band));
    SKH_CHECK(dev_alloc(c, hits, sizeof(skh_hit) * (size_t)band));
    const MtexP mtexp = make_mtex(c);
    for (uint64_t first = 0; first < total; first += band)
    {
        ap.first = (uint32_t)first, ap.count = (uint32_t)std::min<uint64_t>(band, total - first);
        {
            SpanGuard g(c, KC_AOV);
            k_aov_raygen<<<(ap.count + 255) / 256, 256, 0, c->dev.stream>>>(ap, rays.as<float4>());
        }
        SKH_CHECK(trace_device_as(c, rays.p, ap.count, SKH_TRACE_CLOSEST, hits.p, 1, KC_AOV));
        AovPlanes out;
        for (uint32_t k = 0; k < SKH_AOV_COUNT; ++k)
            out.p[k] = ((planes >> k) & 1u) ? reinterpret_cast<uint4*>(d_planes[k]) + first : nullptr;
        {
            SpanGuard g(c, KC_AOV);
            k_aov_resolve<<<(ap.count + 255) / 256, 256, 0, c->dev.stream>>>(make_dev_scene(c), mtexp, ap, planes, rays.as<float4>(), hits.as<skh_hit>(), out);
        }
        SKH_TRY(c, hipGetLastError());
        SKH_TRY(c, hipStreamSynchronize(c->dev.stream)); // (the band's buffers are reused)
    }
    if (c->opt.timing)
        harvest_spans(c);
    c->aov.info.calls++;
    c->aov.info.rays += total;
    c->aov.info.ms_last = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->aov.info.bytes_last = 16ull * total * (uint64_t)__builtin_popcount(planes);
    return SKH_OK;
}

skh_status skh_get_aov_info(skh_context* c, skh_aov_info* out)
{
    return get_info(c, &skh_context::aov, out);
}

// ---- skh_set_option: one row per name ----
// What setting an option costs beyond the store.  OPT_REBUILD: a hierarchy depends on it -- the build is invalidated, and with it skh_update_accel's in-place
// path (include/strelka_hip.h).  OPT_FRAME: the frame's buffers are sized by it -- they are allocated again when a frame exists.
enum OptEffect
{
    OPT_NONE,
    OPT_REBUILD,
    OPT_FRAME
};
struct OptRow
{
    const char* name;
    int64_t lo, hi; // accepted range, inclusive
    OptEffect effect;
    void (*store)(skh_context*, int64_t);
    bool needsSegNode = false;            // value 1 is refused by a library compiled without segment-node support (skh_kernels.h SKH_SEGNODE)
    bool skh_context::Options::*counters = nullptr; // timing / count_traversal: speculation is dropped only when the flag CHANGES (and the last parameters are kept)
};
static const int64_t kOptMin = INT64_MIN, kOptMax = INT64_MAX; // (kOptMin .. kOptMax: any value, read as value != 0)
#define OPT_U32(field) [](skh_context* c, int64_t v) { c->opt.field = (uint32_t)v; }
#define OPT_I32(field) [](skh_context* c, int64_t v) { c->opt.field = (int32_t)v; }
#define OPT_FLAG(field) [](skh_context* c, int64_t v) { c->opt.field = v != 0; }
static const OptRow kOptions[] = {
    // a pass traced ahead with the OTHER setting must not be delivered under this one: its traversal counters would be missing from the
    // per-ray figures while its rays count; the pass in flight is waited for and dropped too
    { "count_traversal", kOptMin, kOptMax, OPT_NONE, OPT_FLAG(countTraversal), false, &skh_context::Options::countTraversal },
    { "timing", kOptMin, kOptMax, OPT_NONE, OPT_FLAG(timing), false, &skh_context::Options::timing },
    // (an explicitly set value applies to the curve build too: its own defaults hold until then)
    { "fetch_min_closest", 1, 64, OPT_NONE, [](skh_context* c, int64_t v) { c->opt.fetchMinClosestSet = true, c->opt.fetchMinClosest = c->opt.curveFetchMinClosest = (uint32_t)v; } },
    { "fetch_min_shadow", 1, 64, OPT_NONE, [](skh_context* c, int64_t v) { c->opt.fetchMinShadow = c->opt.curveFetchMinShadow = (uint32_t)v; } },
    { "node_break_closest", 0, 64, OPT_NONE, [](skh_context* c, int64_t v) { c->opt.nodeBreakClosest = c->opt.curveNodeBreakClosest = (uint32_t)v; } },
    { "node_break_shadow", 0, 64, OPT_NONE, [](skh_context* c, int64_t v) { c->opt.nodeBreakShadow = c->opt.curveNodeBreakShadow = (uint32_t)v; } },
    { "curve_min", 1, 64, OPT_NONE, [](skh_context* c, int64_t v) { c->opt.curveMin = c->opt.worldCurveMin = (uint32_t)v; } },
    { "fetch_min_closest_small", 1, 64, OPT_NONE, OPT_U32(fetchMinClosestSmall) },
    { "fetch_chunk", -1, 4096, OPT_NONE, OPT_I32(fetchChunk) },
    { "leaf_min", 0, 64, OPT_NONE, OPT_U32(leafMin) },
    { "overlap", 0, 2, OPT_NONE, OPT_I32(overlap) },
    { "tail_split", -1, 2, OPT_NONE, OPT_I32(tailSplit) },
    { "small_waves_first", 0, 64, OPT_NONE, OPT_U32(smallWavesFirst) },
    { "small_waves_last", 0, 64, OPT_NONE, OPT_U32(smallWavesLast) },
    { "small_waves_closest", 0, 64, OPT_NONE, OPT_U32(smallWavesClosest) },
    { "small_waves_shadow", 0, 64, OPT_NONE, OPT_U32(smallWavesShadow) },
    { "env_nee", 0, 1, OPT_NONE, OPT_U32(envNee) },
    { "emit_nee", 0, 1, OPT_NONE, OPT_U32(emitNee) },
    { "cutout_rounds", 1, 32, OPT_NONE, OPT_U32(cutoutRounds) }, // (the frame's counter words are sized by it: cut_alloc_frame before the next render)
    { "aov_band", 64, 1 << 26, OPT_NONE, OPT_U32(aovBand) },
    { "speculate", 0, 64, OPT_NONE, OPT_U32(speculateMax) },
    { "speculate_grow", 2, 64, OPT_NONE, OPT_U32(speculateGrow) },
    { "speculate_async", 0, 1, OPT_NONE, [](skh_context* c, int64_t v) { spec_drop(c), c->opt.speculateAsync = (uint32_t)v; } },
    { "world_kernel", kOptMin, kOptMax, OPT_NONE, OPT_FLAG(worldKernel) }, // (the build reads it -- worldCurveKernel -- and setting it has never invalidated the build)
    // the frame's buffers
    { "subframe_batch", 0, 64, OPT_FRAME, OPT_U32(subframeBatch) },
    // where the camera rays go in the first queue (skh_order.h): read by the next pass, which builds the tables it finds missing
    { "queue_order", 0, 1, OPT_NONE, OPT_U32(queueOrder) },
    { "cell_blocks", -1, 64, OPT_NONE, OPT_I32(cellBlocks) },
    { "waves_per_cu", 1, 32, OPT_FRAME, OPT_U32(wavesPerCU) },
    { "waves_per_cu_shadow", 1, 32, OPT_FRAME, OPT_U32(wavesPerCUShadow) },
    { "waves_per_cu_world", 1, 32, OPT_FRAME, OPT_U32(wavesPerCUWorld) },
    { "waves_per_cu_shadow_world", 1, 32, OPT_FRAME, OPT_U32(wavesPerCUShadowWorld) },
    // what skh_build_accel reads
    { "compact_hits", 0, 1, OPT_REBUILD, OPT_U32(compactHits) }, // (skh_build_accel decides with it which word a baked triangle's hit carries)
    { "direct_records", -1, 1, OPT_REBUILD, OPT_I32(directRecords) },
    { "merge_light_proxies", 0, 1, OPT_REBUILD, OPT_U32(mergeLightProxies) },
    { "tight_instance_boxes", kOptMin, kOptMax, OPT_REBUILD, OPT_FLAG(tightInstanceBoxes) },
    { "curve_leaf", 1, 4, OPT_REBUILD, OPT_U32(curveLeaf) },
    { "split_pairs", 0, 1000, OPT_REBUILD, OPT_U32(splitPairs) },
    { "curve_merge", 0, 1, OPT_REBUILD, OPT_U32(curveMerge) },
    { "curve_segnode", 0, 1, OPT_REBUILD, OPT_U32(curveSegNode), true },
    { "curve_strand_major", 0, 1, OPT_REBUILD, OPT_U32(curveStrandMajor), true },
    { "curve_split", 1, 8, OPT_REBUILD, OPT_U32(curveSplit) },
    { "tlas_build", 0, 2, OPT_REBUILD, OPT_U32(tlasBuild) },
    { "tlas_open", 0, 64, OPT_REBUILD, OPT_U32(tlasOpen) },
    { "bake_world", 0, 4, OPT_REBUILD, OPT_U32(bakeWorld) },
    { "bake_budget_mtris", 0, 100, OPT_REBUILD, OPT_U32(bakeBudgetMTris) }, // (leaf references address 2^27 baked triangles)
    { "bake_small_tris", 0, 1 << 20, OPT_REBUILD, OPT_U32(bakeSmallTris) },
    { "morton_bits", 4, 21, OPT_REBUILD, OPT_U32(mortonBits) },
    { "leaf_lines", 0, 1, OPT_REBUILD, OPT_U32(leafLines) },
    { "leaf_max_tris", 1, 8, OPT_REBUILD, OPT_U32(leafMaxTris) },
    { "build_quality", kOptMin, kOptMax, OPT_REBUILD, OPT_FLAG(buildQuality) },
    { "reinsert_rounds", 0, 64, OPT_REBUILD, OPT_U32(reinsertRounds) },
    { "reinsert_curve_rounds", 0, 64, OPT_REBUILD, OPT_U32(reinsertCurveRounds) },
    { "reinsert_min_size", 0, 1 << 24, OPT_REBUILD, OPT_U32(reinsertMinSize) },
    { "ploc_top", 0, kOptMax, OPT_REBUILD, OPT_U32(plocTop) },
};
#undef OPT_U32
#undef OPT_I32
#undef OPT_FLAG

skh_status skh_set_option(skh_context* c, const char* name, int64_t value)
{
    if (!c || !name)
        return SKH_INVALID_ARGUMENT;
    const OptRow* row = nullptr;
    for (const OptRow& r : kOptions)
        if (strcmp(r.name, name) == 0)
            row = &r;
    if (!row || !row->counters)
        spec_drop(c);
    else if (c->opt.*(row->counters) != (value != 0))
        spec_drop(c, true);
    if (!row)
    {
        c->dev.err = std::string("skh_set_option: unknown option ") + name;
        return SKH_INVALID_ARGUMENT;
    }
    if (value < row->lo || value > row->hi || (row->needsSegNode && value == 1 && !SKH_SEGNODE))
        return SKH_INVALID_ARGUMENT;
    row->store(c, value);
    if (row->effect == OPT_REBUILD)
        touched(c, skh_stale::IN_REBUILD_OPTION);
    if (row->effect == OPT_FRAME && c->frame.width)
        return alloc_frame(c);
    return SKH_OK;
}

skh_status skh_get_device_info(skh_context* c, skh_device_info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    hipDeviceProp_t prop;
    SKH_TRY(c, hipGetDeviceProperties(&prop, c->dev.device));
    memset(out, 0, sizeof(*out));
    out->compute_units = (uint32_t)prop.multiProcessorCount;
    out->simds_per_cu = 4;
    out->clock_khz = (uint32_t)prop.clockRate;
    out->memory_clock_khz = (uint32_t)prop.memoryClockRate;
    out->memory_bus_bits = (uint32_t)prop.memoryBusWidth;
    out->wavefront_size = (uint32_t)prop.warpSize;
    out->total_memory_bytes = (uint64_t)prop.totalGlobalMem;
    strncpy(out->name, prop.name, sizeof(out->name) - 1);
    return SKH_OK;
}

skh_status skh_get_build_info(skh_context* c, skh_build_info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    *out = c->accel.buildInfo;
    out->ms_build = c->accel.msBuild;
    return SKH_OK;
}

skh_status skh_get_stats(skh_context* c, skh_stats* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    StatsDev sd;
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    SKH_TRY(c, hipMemcpy(&sd, c->timing.dStats.p, sizeof(sd), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    // rays count when their sub-frame is DELIVERED: what was traced ahead and thrown away (spec_drop) is out, and so is what is still
    // waiting to be collected -- the rest of the current pass and the whole pass in flight (complete after the synchronize above)
    uint64_t outR = c->spec.discardedRadiance, outS = c->spec.discardedShadow;
    {
        const skh_context::Speculation& sp = c->spec;
        if (sp.valid && sp.consumed < sp.count && sp.count > 0)
        {
            outR += sp.passRadiance * (sp.count - sp.consumed) / sp.count;
            outS += sp.passShadow * (sp.count - sp.consumed) / sp.count;
        }
        if (sp.nextInFlight)
        {
            outR += sd.raysRadiance - std::min<uint64_t>(sd.raysRadiance, sp.statsMark[0]);
            outS += sd.raysShadow - std::min<uint64_t>(sd.raysShadow, sp.statsMark[1]);
        }
    }
    out->rays_radiance = sd.raysRadiance - std::min<uint64_t>(sd.raysRadiance, outR);
    out->rays_shadow = sd.raysShadow - std::min<uint64_t>(sd.raysShadow, outS);
    out->speculated_discarded = c->spec.discardedSubframes;
    for (int k = 0; k < 2; ++k)
    {
        out->nodes_visited[k] = sd.nodes[k];
        out->prims_tested[k] = sd.prims[k];
        out->segs_tested[k] = sd.segs[k];
        out->instances_entered[k] = sd.insts[k];
    }
#ifdef SKH_LANE_PROFILE
    for (int k = 0; k < 2; ++k)
        fprintf(stderr, "[lane-profile] %s: rays %llu nodes %llu (TLAS %llu) tris %llu insts %llu | wave: nodeIt %llu triIt %llu instBlk %llu outer %llu refills %llu refilled %llu | tri passes with: fp64 fallback %llu, sign test passed %llu, division %llu | curve blocks %llu (instBlk = Newton runs in the curve builds)\n",
                k ? "shadow" : "closest", k ? sd.raysShadow : sd.raysRadiance, sd.nodes[k], sd.segs[k], sd.prims[k], sd.insts[k], sd.wave[k][0], sd.wave[k][1],
                sd.wave[k][2], sd.wave[k][3], sd.wave[k][4], sd.wave[k][5], sd.wave[k][6], sd.wave[k][8], sd.wave[k][7], sd.wave[k][9]);
    {
        double tot = 0;
        for (int k = 0; k < 8; ++k)
            tot += (double)sd.shade[k];
        fprintf(stderr, "[shade-cycles] load %.1f%% hit+material %.1f%% bsdf_sample %.1f%% light %.1f%% bsdf_eval %.1f%% rest-of-hit %.1f%% tail+state %.1f%% compaction+queues %.1f%%\n",
                100 * sd.shade[0] / tot, 100 * sd.shade[1] / tot, 100 * sd.shade[2] / tot, 100 * sd.shade[3] / tot, 100 * sd.shade[4] / tot, 100 * sd.shade[5] / tot,
                100 * sd.shade[6] / tot, 100 * sd.shade[7] / tot);
    }
    fprintf(stderr, "[slow-rays] %u rays took more than 1500 node steps\n", sd.slowCount);
    for (uint32_t k = 0; k < std::min(sd.slowCount, 16u); ++k)
        fprintf(stderr, "[slow-ray] steps %.0f tris %.0f insts %.0f %s o %.9g %.9g %.9g d %.9g %.9g %.9g tmin %g tmax %g\n", sd.slow[k][0], sd.slow[k][1], sd.slow[k][2],
                sd.slow[k][3] != 0.0f ? "shadow" : "closest", sd.slow[k][4], sd.slow[k][5], sd.slow[k][6], sd.slow[k][7], sd.slow[k][8], sd.slow[k][9], sd.slow[k][10], sd.slow[k][11]);
    for (int k = 0; k < 2; ++k)
    {
        unsigned long long tr = 0, tb = 0;
        for (int j = 0; j < 42; ++j)
            tr += sd.runHist[k][j], tb += sd.blockHist[k][j];
        if (tr)
        {
            fprintf(stderr, "[newton-steps] %s runs %llu:", k ? "shadow" : "closest", tr);
            for (int j = 0; j < 42; ++j)
                fprintf(stderr, " %d:%.2f%%", j, 100.0 * (double)sd.runHist[k][j] / (double)tr);
            fprintf(stderr, "\n[newton-block-max] %s rounds %llu:", k ? "shadow" : "closest", tb);
            for (int j = 0; j < 42; ++j)
                fprintf(stderr, " %d:%.2f%%", j, 100.0 * (double)sd.blockHist[k][j] / (double)tb);
            fprintf(stderr, "\n");
        }
    }
    for (int k = 0; k < 2; ++k)
        fprintf(stderr, "[lane-cycles] %s: refill %.3g curve-block %.3g node %.3g leaf %.3g pop %.3g write %.3g total %.3g | shader clock while the waves ran: %.1f MHz (wave-seconds %.4g)\n", k ? "shadow" : "closest", (double)sd.cyc[k][0], (double)sd.cyc[k][8],
                (double)sd.cyc[k][1], (double)sd.cyc[k][2], (double)sd.cyc[k][3], (double)sd.cyc[k][4], (double)sd.cyc[k][5],
                sd.cyc[k][7] ? (double)sd.cyc[k][6] / (double)sd.cyc[k][7] * 100.0 : 0.0, (double)sd.cyc[k][7] / 1e8);
#endif
#ifdef SKH_TAIL_PROFILE
    for (int k = 0; k < 2; ++k)
    {
        unsigned long long waves = 0;
        double liveSum = 0;
        for (int j = 0; j < 64; ++j)
            waves += sd.exitHist[k][j];
        for (int j = 0; j < 65; ++j)
            liveSum += (double)j * (double)sd.dryLive[k][j];
        if (!waves)
            continue;
        fprintf(stderr, "[launch-tail] %s: %llu waves; lanes alive at a wave's dry point: mean %.1f; after it a wave stays %.1f us and spends %.1f ray-us (= %.1f lanes alive on average)\n", k ? "shadow" : "closest",
                waves, liveSum / (double)waves, (double)sd.waveTicksAfterDry[k] / 100.0 / (double)waves, (double)sd.rayTicksAfterDry[k] / 100.0 / (double)waves,
                sd.waveTicksAfterDry[k] ? (double)sd.rayTicksAfterDry[k] / (double)sd.waveTicksAfterDry[k] : 0.0);
        fprintf(stderr, "[launch-tail]   16-us bins: from the launch's first wave -- waves finding the queue dry %%, waves leaving %% | from a wave's own dry point -- waves leaving %%\n");
        for (int j = 0; j < 64; ++j)
            if (sd.dryHist[k][j] || sd.exitHist[k][j] || sd.afterDryHist[k][j])
                fprintf(stderr, "[launch-tail]   %4d us: dry %5.1f%%  exit %5.1f%% | exit after dry %5.1f%%\n", 16 * j, 100.0 * (double)sd.dryHist[k][j] / (double)waves, 100.0 * (double)sd.exitHist[k][j] / (double)waves,
                        100.0 * (double)sd.afterDryHist[k][j] / (double)waves);
    }
#endif
    out->ms_trace_closest = c->timing.msClass[KC_TRACE_CLOSEST];
    out->ms_trace_shadow = c->timing.msClass[KC_TRACE_SHADOW];
    out->ms_shade = c->timing.msClass[KC_SHADE];
    out->ms_raygen = c->timing.msClass[KC_RAYGEN];
    out->ms_accumulate = c->timing.msClass[KC_ACCUM];
    out->ms_sort = c->timing.msClass[KC_SORT];
    out->ms_build = c->accel.msBuild;
    out->launches_trace_closest = c->timing.launches[KC_TRACE_CLOSEST];
    out->launches_trace_shadow = c->timing.launches[KC_TRACE_SHADOW];
    out->launches_shade = c->timing.launches[KC_SHADE];
    out->launches_other = c->timing.launches[KC_RAYGEN] + c->timing.launches[KC_ACCUM];
    out->stack_overflows = c->timing.stackOverflows;
    return SKH_OK;
}

skh_status skh_reset_stats(skh_context* c)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    spec_drop(c, true); // (what was traced ahead belongs to the counters being cleared)
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    SKH_TRY(c, hipMemset(c->timing.dStats.p, 0, sizeof(StatsDev)));
    SKH_TRY(c, hipMemset(c->cut.dStats.p, 0, sizeof(CutStatsDev)));
    c->timing.stackOverflows = 0;
    c->spec.discardedRadiance = c->spec.discardedShadow = 0;
    c->spec.discardedSubframes = 0;
    c->aov.info.calls = c->aov.info.rays = 0;
    c->dn.info.calls = c->dn.info.pixels = 0;
    c->tp.info.calls = c->tp.info.pixels = 0;
    c->mo.info.calls = c->mo.info.pixels = 0;
    c->vd.info.calls = c->vd.info.pixels = 0;
    c->rw.info.calls = c->rw.info.pixels = 0;
    c->rc.info.calls = c->rc.info.pixels = 0;
    for (int k = 0; k < KC_COUNT; ++k)
    {
        c->timing.msClass[k] = 0.0;
        c->timing.launches[k] = 0;
    }
    return SKH_OK;
}

skh_status skh_synchronize(skh_context* c)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}

void* skh_get_stream(skh_context* c)
{
    return c ? (void*)c->dev.stream : nullptr;
}

