// skh_image.inc -- host side of the image passes: the passes over caller-owned image planes that follow a render (skh_denoise, skh_temporal, skh_moments,
// skh_denoise_variance, skh_rewind_guides, skh_rectify; their kernels: skh_image.h and the five headers that include it).
// Included by strelka_hip.hip (one translation unit); needs skh_host.h and side_stream above it.
//
// A new pass costs one kernel body, one refusal function and one entry point written around ImagePass.

// ---- what the passes share ----
// What an entry point of an image pass is written around.  The constructor sets the device; begin(why) leaves the message of a refusal, or notes the time and
// hands out the stream (beside a pass traced ahead, not behind it: skh_tonemap's choice); end() checks the launches, waits for them and keeps the call's figures.
struct ImagePass
{
    skh_context* c;
    const char* fn;
    hipStream_t st = nullptr;
    std::chrono::steady_clock::time_point t0;

    ImagePass(skh_context* ctx, const char* name) : c(ctx), fn(name)
    {
        (void)hipSetDevice(c->dev.device);
    }
    skh_status begin(const char* why)
    {
        if (why)
        {
            c->dev.err = std::string(fn) + ": " + why;
            return SKH_INVALID_ARGUMENT;
        }
        t0 = std::chrono::steady_clock::now();
        st = side_stream(c);
        return SKH_OK;
    }
    skh_status tried(hipError_t e, const char* call) // (SKH_TRY under the entry point's name)
    {
        if (e == hipSuccess)
            return SKH_OK;
        c->dev.err = std::string(fn) + ": " + call + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? SKH_OUT_OF_MEMORY : SKH_FAIL;
    }
    template <typename Info>
    skh_status end(Info& info, uint64_t pixels)
    {
        SKH_CHECK(tried(hipGetLastError(), "hipGetLastError()"));
        SKH_CHECK(tried(hipStreamSynchronize(st), "hipStreamSynchronize(st)"));
        info.calls++;
        info.pixels += pixels;
        info.ms_last = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return SKH_OK;
    }
};

// the pieces of a refusal: why the value is refused, or nullptr
static const char* size_refusal(uint32_t width, uint32_t height)
{
    return (width == 0u || height == 0u || (uint64_t)width * height > (1ull << 26)) ? "an empty image, or one of more than 2^26 pixels" : nullptr;
}
static const char* levels_refusal(uint32_t first_level, uint32_t levels)
{
    return (levels == 0u || first_level > SKH_DENOISE_MAX_LEVEL || levels > SKH_DENOISE_MAX_LEVEL || first_level + levels > SKH_DENOISE_MAX_LEVEL)
               ? "no level, or a level beyond first_level + levels <= 8"
               : nullptr;
}
static const char* albedo_floor_refusal(float albedo_floor)
{
    return (!std::isfinite(albedo_floor) || !(albedo_floor > 0.0f)) ? "an albedo_floor that is <= 0 or not finite" : nullptr;
}
template <size_t N>
static const char* reserved_refusal(const uint32_t (&reserved)[N])
{
    for (uint32_t r : reserved)
        if (r != 0u)
            return "a non-zero reserved word";
    return nullptr;
}
// (inside a *_refusal function: the first piece that refuses is the answer)
#define SKH_REFUSE(piece)                                                                                                                                      \
    if (const char* _why = (piece))                                                                                                                            \
    return _why

// skh_get_*_info: the figures of the subject `sub` of the context
template <typename Sub, typename Info>
static skh_status get_info(skh_context* c, Sub skh_context::*sub, Info* out)
{
    if (!c || !out)
        return SKH_INVALID_ARGUMENT;
    *out = (c->*sub).info;
    return SKH_OK;
}

// a caller's plane as the records the kernels read and write
static inline const float4* f4(const void* p)
{
    return reinterpret_cast<const float4*>(p);
}
static inline float4* f4(void* p)
{
    return reinterpret_cast<float4*>(p);
}
static inline const uint4* u4(const void* p)
{
    return reinterpret_cast<const uint4*>(p);
}
static inline uint4* u4(void* p)
{
    return reinterpret_cast<uint4*>(p);
}

static const dim3 kImgBlock(64, 4); // (the grid: img_grid, skh_image.h)

// the scratch of the two filters for n pixels: the packed colour image (`second`: and the one it ping-pongs with) and the guide record
static skh_status filter_scratch(skh_context* c, size_t n, bool second)
{
    SKH_CHECK(dev_alloc(c, c->dn.dColor[0], 16 * n));
    if (second)
        SKH_CHECK(dev_alloc(c, c->dn.dColor[1], 16 * n));
    SKH_CHECK(dev_alloc(c, c->dn.dG0, 16 * n));
    SKH_CHECK(dev_alloc(c, c->dn.dG1, 8 * n));
    return SKH_OK;
}
static uint64_t filter_scratch_bytes(const skh_context* c)
{
    return (uint64_t)c->dn.dColor[0].bytes + c->dn.dColor[1].bytes + c->dn.dG0.bytes + c->dn.dG1.bytes;
}

// ---- the denoiser (skh_denoise.h): skh_denoise_check, skh_denoise, skh_get_denoise_info ----
static_assert(sizeof(skh_denoise_params) == 64 && sizeof(skh_denoise_info) == 32, "ABI layout");

// why *p is refused, or nullptr
static const char* denoise_refusal(const skh_denoise_params* p)
{
    if (!p)
        return "no parameters";
    SKH_REFUSE(size_refusal(p->width, p->height));
    SKH_REFUSE(levels_refusal(p->first_level, p->levels));
    for (float s : { p->sigma_color, p->sigma_normal, p->sigma_plane })
        if (!(s > 0.0f)) // (a NaN too)
            return "a sigma that is <= 0 or NaN";
    SKH_REFUSE(albedo_floor_refusal(p->albedo_floor));
    if (p->flags & ~(SKH_DENOISE_DEMODULATE | SKH_DENOISE_REMODULATE))
        return "an unknown flag bit";
    return reserved_refusal(p->reserved);
}

skh_status skh_denoise_check(const skh_denoise_params* p)
{
    return denoise_refusal(p) ? SKH_INVALID_ARGUMENT : SKH_OK;
}

skh_status skh_denoise(skh_context* c, const skh_denoise_params* p, const void* d_color, const void* d_ids, const void* d_normal, const void* d_position,
                       const void* d_albedo, void* d_out)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    ImagePass pass(c, "skh_denoise");
    if (!p) // free the scratch
    {
        dev_free(c->dn.dColor[0]), dev_free(c->dn.dColor[1]), dev_free(c->dn.dG0), dev_free(c->dn.dG1);
        return SKH_OK;
    }
    const char* why = denoise_refusal(p);
    if (!why && (!d_color || !d_ids || !d_normal || !d_position || !d_out))
        why = "a NULL image";
    if (!why && p->flags != 0u && !d_albedo)
        why = "a flag that needs the albedo plane, and no albedo plane";
    SKH_CHECK(pass.begin(why));
    const size_t n = (size_t)p->width * p->height;
    SKH_CHECK(filter_scratch(c, n, p->levels > 1u));
    DnP dp;
    dp.width = p->width, dp.height = p->height, dp.step = 1u, dp.kc = 0.0f;
    dp.kn = 1.0f / (p->sigma_normal * p->sigma_normal), dp.kp = 1.0f / (p->sigma_plane * p->sigma_plane);
    dp.albedoFloor = p->albedo_floor, dp.flags = p->flags;
    const float4* g0 = c->dn.dG0.as<float4>();
    const float2* g1 = c->dn.dG1.as<float2>();
    k_img_pack<false><<<(uint32_t)((n + 255) / 256), 256, 0, pass.st>>>((uint32_t)n, p->flags & SKH_DENOISE_DEMODULATE, p->albedo_floor, f4(d_color), u4(d_ids), f4(d_normal),
                                                                       f4(d_position), f4(d_albedo), nullptr, c->dn.dColor[0].as<float4>(), c->dn.dG0.as<float4>(),
                                                                       c->dn.dG1.as<float2>());
    const dim3 grid = img_grid(p->width, p->height);
    for (uint32_t k = 0; k < p->levels; ++k)
    {
        const uint32_t level = p->first_level + k;
        const float sc = p->sigma_color * (1.0f / (float)(1u << level)); // (exact: a power of two)
        dp.step = 1u << level, dp.kc = 1.0f / (sc * sc);
        const float4* cin = c->dn.dColor[k & 1u].as<float4>();
        if (k + 1u < p->levels)
            k_dn_level<false><<<grid, kImgBlock, 0, pass.st>>>(dp, cin, g0, g1, c->dn.dColor[(k + 1u) & 1u].as<float4>(), nullptr, nullptr, nullptr);
        else
            k_dn_level<true><<<grid, kImgBlock, 0, pass.st>>>(dp, cin, g0, g1, nullptr, u4(d_color), f4(d_albedo), u4(d_out));
    }
    return pass.end(c->dn.info, n);
}

skh_status skh_get_denoise_info(skh_context* c, skh_denoise_info* out)
{
    SKH_CHECK(get_info(c, &skh_context::dn, out));
    out->scratch_bytes = filter_scratch_bytes(c);
    return SKH_OK;
}

// ---- temporal accumulation (skh_temporal.h): skh_temporal_check, skh_temporal, skh_get_temporal_info ----
static_assert(sizeof(skh_temporal_params) == 128 && sizeof(skh_temporal_info) == 24, "ABI layout");

// why *p is refused, or nullptr
static const char* temporal_refusal(const skh_temporal_params* p)
{
    if (!p)
        return "no parameters";
    SKH_REFUSE(size_refusal(p->width, p->height));
    for (float m : p->prev_world_to_clip)
        if (!std::isfinite(m))
            return "a matrix entry that is not finite";
    if (!(p->normal_min >= -1.0f && p->normal_min <= 1.0f)) // (a NaN too)
        return "a normal_min outside [-1, 1] or NaN";
    if (!(p->plane_tolerance > 0.0f))
        return "a plane_tolerance that is <= 0 or NaN";
    if (!std::isfinite(p->max_history) || !(p->max_history >= 1.0f))
        return "a max_history that is < 1 or not finite";
    if (!std::isfinite(p->initial_length) || !(p->initial_length >= 1.0f) || !(p->initial_length <= p->max_history))
        return "an initial_length that is < 1, above max_history or not finite";
    SKH_REFUSE(albedo_floor_refusal(p->albedo_floor));
    if (p->flags & ~SKH_TEMPORAL_DEMODULATE)
        return "an unknown flag bit";
    return reserved_refusal(p->reserved);
}

skh_status skh_temporal_check(const skh_temporal_params* p)
{
    return temporal_refusal(p) ? SKH_INVALID_ARGUMENT : SKH_OK;
}

// the kernels' record of *p; hasPrev: a previous frame is given
static TpP make_temporal(const skh_temporal_params* p, bool hasPrev)
{
    TpP tp;
    tp.width = p->width, tp.height = p->height;
    for (int k = 0; k < 16; ++k)
        tp.prevWorldToClip[k] = p->prev_world_to_clip[k];
    tp.normalMin = p->normal_min, tp.planeTolerance = p->plane_tolerance, tp.maxHistory = p->max_history, tp.initialLength = p->initial_length;
    tp.albedoFloor = p->albedo_floor, tp.flags = p->flags, tp.hasPrev = hasPrev ? 1u : 0u;
    return tp;
}

skh_status skh_temporal(skh_context* c, const skh_temporal_params* p, const void* d_color, const void* d_ids, const void* d_normal, const void* d_position,
                        const void* d_albedo, const void* d_prev_history, const void* d_prev_ids, const void* d_prev_normal, const void* d_prev_position,
                        void* d_out, void* d_history_out, void* d_motion)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    ImagePass pass(c, "skh_temporal");
    const char* why = temporal_refusal(p);
    if (!why && (!d_color || !d_ids || !d_normal || !d_position || !d_out || !d_history_out))
        why = "a NULL image";
    if (!why && (p->flags & SKH_TEMPORAL_DEMODULATE) && !d_albedo)
        why = "a flag that needs the albedo plane, and no albedo plane";
    if (!why && d_prev_history && (!d_prev_ids || !d_prev_normal || !d_prev_position))
        why = "a previous history without its guide planes";
    if (!why && d_prev_history && d_history_out == d_prev_history)
        why = "d_history_out == d_prev_history (taps read neighbours)";
    SKH_CHECK(pass.begin(why));
    k_tp_reproject<<<img_grid(p->width, p->height), kImgBlock, 0, pass.st>>>(make_temporal(p, d_prev_history != nullptr), u4(d_color), u4(d_ids), f4(d_normal),
                                                                            f4(d_position), f4(d_albedo), f4(d_prev_history), u4(d_prev_ids), f4(d_prev_normal),
                                                                            f4(d_prev_position), u4(d_out), f4(d_history_out), f4(d_motion));
    return pass.end(c->tp.info, (uint64_t)p->width * p->height);
}

skh_status skh_get_temporal_info(skh_context* c, skh_temporal_info* out)
{
    return get_info(c, &skh_context::tp, out);
}

// ---- variance guidance (skh_variance.h): skh_moments, skh_get_moments_info, skh_vdenoise_check, skh_denoise_variance, skh_get_vdenoise_info ----
static_assert(sizeof(skh_moments_info) == 24 && sizeof(skh_vdenoise_params) == 64 && sizeof(skh_vdenoise_info) == 32, "ABI layout");

skh_status skh_moments(skh_context* c, const skh_temporal_params* p, const void* d_color, const void* d_ids, const void* d_position, const void* d_albedo,
                       const void* d_motion, const void* d_prev_moments, void* d_moments_out)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    ImagePass pass(c, "skh_moments");
    const char* why = temporal_refusal(p);
    if (!why && (!d_color || !d_ids || !d_position || !d_moments_out))
        why = "a NULL image";
    if (!why && (p->flags & SKH_TEMPORAL_DEMODULATE) && !d_albedo)
        why = "a flag that needs the albedo plane, and no albedo plane";
    if (!why && (d_motion == nullptr) != (d_prev_moments == nullptr))
        why = "exactly one of d_motion and d_prev_moments";
    if (!why && d_prev_moments && d_moments_out == d_prev_moments)
        why = "d_moments_out == d_prev_moments (taps read neighbours)";
    SKH_CHECK(pass.begin(why));
    k_vr_moments<<<img_grid(p->width, p->height), kImgBlock, 0, pass.st>>>(make_temporal(p, d_prev_moments != nullptr), f4(d_color), u4(d_ids), f4(d_position),
                                                                          f4(d_albedo), f4(d_motion), f4(d_prev_moments), f4(d_moments_out));
    return pass.end(c->mo.info, (uint64_t)p->width * p->height);
}

skh_status skh_get_moments_info(skh_context* c, skh_moments_info* out)
{
    return get_info(c, &skh_context::mo, out);
}

// why *p is refused, or nullptr
static const char* vdenoise_refusal(const skh_vdenoise_params* p)
{
    if (!p)
        return "no parameters";
    SKH_REFUSE(size_refusal(p->width, p->height));
    SKH_REFUSE(levels_refusal(p->first_level, p->levels));
    for (float s : { p->sigma_luminance, p->sigma_normal, p->sigma_plane })
        if (!(s > 0.0f)) // (a NaN too)
            return "a sigma that is <= 0 or NaN";
    SKH_REFUSE(albedo_floor_refusal(p->albedo_floor));
    if (!std::isfinite(p->epsilon) || !(p->epsilon > 0.0f))
        return "an epsilon that is <= 0 or not finite";
    if (!std::isfinite(p->min_history) || !(p->min_history >= 1.0f))
        return "a min_history that is < 1 or not finite";
    if (p->flags & ~(SKH_DENOISE_DEMODULATE | SKH_DENOISE_REMODULATE | SKH_VDENOISE_ESTIMATE))
        return "an unknown flag bit";
    return reserved_refusal(p->reserved);
}

skh_status skh_vdenoise_check(const skh_vdenoise_params* p)
{
    return vdenoise_refusal(p) ? SKH_INVALID_ARGUMENT : SKH_OK;
}

skh_status skh_denoise_variance(skh_context* c, const skh_vdenoise_params* p, const void* d_color, const void* d_ids, const void* d_normal,
                                const void* d_position, const void* d_albedo, const void* d_moments, void* d_out, void* d_moments_out)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    if (!p) // free the scratch: skh_denoise's
        return skh_denoise(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    ImagePass pass(c, "skh_denoise_variance");
    const char* why = vdenoise_refusal(p);
    if (!why && (!d_color || !d_ids || !d_normal || !d_position || !d_moments || !d_out))
        why = "a NULL image";
    if (!why && (p->flags & (SKH_DENOISE_DEMODULATE | SKH_DENOISE_REMODULATE)) && !d_albedo)
        why = "a flag that needs the albedo plane, and no albedo plane";
    SKH_CHECK(pass.begin(why));
    const size_t n = (size_t)p->width * p->height;
    const uint32_t est = (p->flags & SKH_VDENOISE_ESTIMATE) ? 1u : 0u;
    SKH_CHECK(filter_scratch(c, n, p->levels + est > 1u));
    VrP vp;
    vp.width = p->width, vp.height = p->height, vp.step = 1u;
    vp.lumOff = std::isinf(p->sigma_luminance) ? 1u : 0u;
    vp.sigmaLuminance = vp.lumOff ? 0.0f : p->sigma_luminance, vp.epsilon = p->epsilon;
    vp.kn = 1.0f / (p->sigma_normal * p->sigma_normal), vp.kp = 1.0f / (p->sigma_plane * p->sigma_plane);
    vp.albedoFloor = p->albedo_floor, vp.minHistory = p->min_history, vp.flags = p->flags;
    const float4* g0 = c->dn.dG0.as<float4>();
    const float2* g1 = c->dn.dG1.as<float2>();
    k_img_pack<true><<<(uint32_t)((n + 255) / 256), 256, 0, pass.st>>>((uint32_t)n, p->flags & SKH_DENOISE_DEMODULATE, p->albedo_floor, f4(d_color), u4(d_ids), f4(d_normal),
                                                                      f4(d_position), f4(d_albedo), f4(d_moments), c->dn.dColor[0].as<float4>(), c->dn.dG0.as<float4>(),
                                                                      c->dn.dG1.as<float2>());
    const dim3 grid = img_grid(p->width, p->height);
    if (est)
        k_vr_estimate<<<grid, kImgBlock, 0, pass.st>>>(vp, c->dn.dColor[0].as<float4>(), g0, g1, f4(d_moments), c->dn.dColor[1].as<float4>());
    for (uint32_t k = 0; k < p->levels; ++k)
    {
        vp.step = 1u << (p->first_level + k);
        const float4* cin = c->dn.dColor[(k + est) & 1u].as<float4>();
        if (k + 1u < p->levels)
            k_vr_level<false><<<grid, kImgBlock, 0, pass.st>>>(vp, cin, g0, g1, c->dn.dColor[(k + est + 1u) & 1u].as<float4>(), nullptr, nullptr, nullptr, nullptr, nullptr);
        else
            k_vr_level<true><<<grid, kImgBlock, 0, pass.st>>>(vp, cin, g0, g1, nullptr, u4(d_color), f4(d_albedo), u4(d_out), f4(d_moments), f4(d_moments_out));
    }
    return pass.end(c->vd.info, n);
}

skh_status skh_get_vdenoise_info(skh_context* c, skh_vdenoise_info* out)
{
    SKH_CHECK(get_info(c, &skh_context::vd, out));
    out->scratch_bytes = filter_scratch_bytes(c);
    return SKH_OK;
}

// ---- object motion (skh_motion.h): skh_instance_motion_from_transforms, skh_instance_motion_check, skh_set_instance_motion, skh_rewind_guides ----
static_assert(sizeof(skh_instance_motion) == 96 && sizeof(skh_rewind_info) == 32, "ABI layout");

// inverse of the row-major 3 x 3 `m` by adjugate / determinant, in the operation order the header writes out; false when the determinant is 0 or not finite
static bool motion_inverse(const double m[3][3], double inv[3][3])
{
    double adj[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            adj[i][j] = m[(j + 1) % 3][(i + 1) % 3] * m[(j + 2) % 3][(i + 2) % 3] - m[(j + 1) % 3][(i + 2) % 3] * m[(j + 2) % 3][(i + 1) % 3];
    const double det = (m[0][0] * adj[0][0] + m[0][1] * adj[1][0]) + m[0][2] * adj[2][0];
    if (det == 0.0 || !std::isfinite(det))
        return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            inv[i][j] = adj[i][j] / det;
    return true;
}

skh_status skh_instance_motion_from_transforms(const float prev[12], const float cur[12], skh_instance_motion* out)
{
    if (!prev || !cur || !out)
        return SKH_INVALID_ARGUMENT;
    skh_instance_motion e = {};
    e.to_prev[0] = e.to_prev[5] = e.to_prev[10] = 1.0f;
    e.normal_to_prev[0] = e.normal_to_prev[4] = e.normal_to_prev[8] = 1.0f;
    if (std::memcmp(prev, cur, 12 * sizeof(float)) == 0)
    {
        *out = e; // flags 0: the entry is skipped
        return SKH_OK;
    }
    skh_instance_motion moved = e;
    bool ok = true;
    double A[3][3], B[3][3], a[3], b[3], Ai[3][3], Bi[3][3];
    for (int i = 0; i < 3; ++i)
    {
        for (int j = 0; j < 3; ++j)
            A[i][j] = prev[4 * i + j], B[i][j] = cur[4 * i + j];
        a[i] = prev[4 * i + 3], b[i] = cur[4 * i + 3];
    }
    for (int k = 0; k < 12; ++k)
        ok = ok && std::isfinite(prev[k]) && std::isfinite(cur[k]);
    ok = ok && motion_inverse(B, Bi) && motion_inverse(A, Ai);
    if (ok)
        for (int i = 0; i < 3; ++i)
        {
            double L[3];
            for (int j = 0; j < 3; ++j)
            {
                L[j] = (A[i][0] * Bi[0][j] + A[i][1] * Bi[1][j]) + A[i][2] * Bi[2][j];
                moved.to_prev[4 * i + j] = (float)L[j];
                const double K = (Ai[0][i] * B[j][0] + Ai[1][i] * B[j][1]) + Ai[2][i] * B[j][2];
                moved.normal_to_prev[3 * i + j] = (float)K;
            }
            moved.to_prev[4 * i + 3] = (float)(a[i] - ((L[0] * b[0] + L[1] * b[1]) + L[2] * b[2]));
        }
    for (int k = 0; ok && k < 12; ++k)
        ok = std::isfinite(moved.to_prev[k]);
    for (int k = 0; ok && k < 9; ++k)
        ok = std::isfinite(moved.normal_to_prev[k]);
    if (ok)
        moved.flags = SKH_MOTION_MOVED, *out = moved;
    else
        e.flags = SKH_MOTION_MOVED | SKH_MOTION_DROP, *out = e;
    return SKH_OK;
}

// why the table is refused, or nullptr
static const char* motion_refusal(const skh_instance_motion* table, uint32_t n)
{
    if (n > 0u && !table)
        return "no table for n > 0";
    for (uint32_t i = 0; i < n; ++i)
    {
        const skh_instance_motion& e = table[i];
        if (e.flags & ~(SKH_MOTION_MOVED | SKH_MOTION_DROP))
            return "an unknown flag bit";
        if ((e.flags & SKH_MOTION_DROP) && !(e.flags & SKH_MOTION_MOVED))
            return "DROP without MOVED";
        if (e.reserved[0] != 0u || e.reserved[1] != 0u)
            return "a non-zero reserved word";
        if (e.flags == SKH_MOTION_MOVED)
        {
            for (float m : e.to_prev)
                if (!std::isfinite(m))
                    return "a matrix word that is not finite in a moved entry";
            for (float m : e.normal_to_prev)
                if (!std::isfinite(m))
                    return "a matrix word that is not finite in a moved entry";
        }
    }
    return nullptr;
}

skh_status skh_instance_motion_check(const skh_instance_motion* table, uint32_t n)
{
    return motion_refusal(table, n) ? SKH_INVALID_ARGUMENT : SKH_OK;
}

skh_status skh_set_instance_motion(skh_context* c, const skh_instance_motion* table, uint32_t n)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (const char* why = motion_refusal(table, n))
    {
        c->dev.err = std::string("skh_set_instance_motion: ") + why;
        return SKH_INVALID_ARGUMENT;
    }
    if (n == 0u)
    {
        dev_free(c->rw.dTable);
        c->rw.entries = 0;
        return SKH_OK;
    }
    c->rw.entries = 0; // (until the new table is in place: a failed upload leaves none)
    SKH_CHECK(dev_upload(c, c->rw.dTable, table, sizeof(skh_instance_motion) * (size_t)n));
    c->rw.entries = n;
    return SKH_OK;
}

skh_status skh_rewind_guides(skh_context* c, uint32_t width, uint32_t height, const void* d_ids, const void* d_position, const void* d_normal, void* d_position_out,
                             void* d_normal_out)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    ImagePass pass(c, "skh_rewind_guides");
    const char* why = size_refusal(width, height);
    if (!why && (!d_ids || !d_position || !d_normal || !d_position_out || !d_normal_out))
        why = "a NULL plane";
    if (!why && (c->rw.entries == 0u || !c->rw.dTable.p))
        why = "no motion table set (skh_set_instance_motion)";
    SKH_CHECK(pass.begin(why));
    k_mo_rewind<<<img_grid(width, height), kImgBlock, 0, pass.st>>>(width, height, c->rw.entries, c->rw.dTable.as<float4>(), u4(d_ids), f4(d_position), f4(d_normal),
                                                                   f4(d_position_out), f4(d_normal_out));
    return pass.end(c->rw.info, (uint64_t)width * height);
}

skh_status skh_get_rewind_info(skh_context* c, skh_rewind_info* out)
{
    SKH_CHECK(get_info(c, &skh_context::rw, out));
    out->entries = c->rw.entries;
    return SKH_OK;
}

// ---- history rectification (skh_rectify.h): skh_rectify_check, skh_rectify, skh_get_rectify_info ----
static_assert(sizeof(skh_rectify_params) == 56 && sizeof(skh_rectify_info) == 24, "ABI layout");

// why *p is refused, or nullptr
static const char* rectify_refusal(const skh_rectify_params* p)
{
    if (!p)
        return "no parameters";
    SKH_REFUSE(size_refusal(p->width, p->height));
    if (p->radius < 1u || p->radius > 3u)
        return "a radius outside 1 ... 3";
    if (!(p->k > 0.0f)) // (a NaN too; +inf is legal)
        return "a k that is <= 0 or NaN";
    SKH_REFUSE(albedo_floor_refusal(p->albedo_floor));
    if (p->flags & ~(SKH_RECTIFY_REMODULATE | SKH_RECTIFY_SHORTEN))
        return "an unknown flag bit";
    return reserved_refusal(p->reserved);
}

skh_status skh_rectify_check(const skh_rectify_params* p)
{
    return rectify_refusal(p) ? SKH_INVALID_ARGUMENT : SKH_OK;
}

skh_status skh_rectify(skh_context* c, const skh_rectify_params* p, const void* d_image, const void* d_ids, const void* d_albedo, const void* d_history,
                       const void* d_fast, void* d_out, void* d_history_out, void* d_info)
{
    if (!c)
        return SKH_INVALID_ARGUMENT;
    ImagePass pass(c, "skh_rectify");
    const char* why = rectify_refusal(p);
    if (!why && (!d_image || !d_ids || !d_history || !d_fast || !d_out || !d_history_out))
        why = "a NULL image";
    if (!why && (p->flags & SKH_RECTIFY_REMODULATE) && !d_albedo)
        why = "a flag that needs the albedo plane, and no albedo plane";
    if (!why && (d_history_out == d_fast || d_out == d_fast))
        why = "an output that is d_fast (the window reads neighbours)";
    SKH_CHECK(pass.begin(why));
    RcP rp;
    rp.width = p->width, rp.height = p->height, rp.k = p->k, rp.albedoFloor = p->albedo_floor, rp.flags = p->flags, rp.kInf = std::isinf(p->k) ? 1u : 0u;
    const auto kernel = p->radius == 1u ? k_rc_rectify<1> : p->radius == 2u ? k_rc_rectify<2> : k_rc_rectify<3>;
    kernel<<<img_grid(p->width, p->height), kImgBlock, 0, pass.st>>>(rp, u4(d_image), u4(d_ids), f4(d_albedo), u4(d_history), f4(d_fast), u4(d_out), u4(d_history_out),
                                                                    f4(d_info));
    return pass.end(c->rc.info, (uint64_t)p->width * p->height);
}

skh_status skh_get_rectify_info(skh_context* c, skh_rectify_info* out)
{
    return get_info(c, &skh_context::rc, out);
}
