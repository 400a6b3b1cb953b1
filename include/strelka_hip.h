/*
 * strelka_hip.h -- C ABI of the MI355X-native wavefront path tracer that sits behind
 * Strelka's oka::Render interface.
 *
 * This header is the drop-in boundary.  Every entry point names the reference interface it
 * replaces (paths relative to the arhix52/Strelka tree).  The ABI is plain C: opaque handle,
 * POD structs, host pointers + counts, int status (0 = ok).  No STL, no glm, no torch types.
 *
 * Ownership: the library owns all device memory.  The caller owns every host pointer it passes;
 * pointers only need to live for the duration of the call.  Device pointers passed in
 * (skh_render_subframe's d_image, skh_copy_accum's d_dst) are caller-owned HBM buffers.
 *
 * Threading: one context per GPU, externally synchronised (same contract as oka::Render, whose
 * render() is synchronous and not re-entrant: src/render/optix/OptixRender.cpp:874-1057).
 *
 * Errors: functions return skh_status; skh_last_error() gives the message.  The library never
 * aborts (the reference logs + assert(0): OptixRender.cpp:61-103).
 */
#ifndef STRELKA_HIP_H
#define STRELKA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKH_ABI_VERSION 5 /* 5 (round 6): + skh_refit_accel, skh_build_info.refit / ms_refit, then skh_update_accel (additive: refit = 2), then skh_set_environment / _transform / skh_get_environment_info + two unit probes (additive), then skh_set_emission / skh_get_emitter_info / skh_emitter_probe (additive), then skh_set_material_blend / skh_get_blend_info / skh_blend_probe (additive), then skh_set_light_shapes / skh_get_light_shape_info / skh_light_shape_probe (additive), then skh_adaptive_check / skh_set_adaptive / skh_get_adaptive_info / skh_read_adaptive (additive), then skh_aov_check / skh_render_aovs / skh_get_aov_info (additive; option aov_band); options curve_merge, curve_segnode, curve_strand_major, split_pairs.  4 (round 5): + skh_get_build_info; options reinsert_rounds, reinsert_min_size; wide, tail_park, tail_lag removed.  3 (round 4): + skh_unit_probe, skh_copy_aov */

/* mirrors oka::Result (include/render/common.h:30-35) */
typedef enum skh_status
{
    SKH_OK = 0,
    SKH_FAIL = 1,
    SKH_OUT_OF_MEMORY = 2,
    SKH_INVALID_ARGUMENT = 3
} skh_status;

typedef struct skh_context skh_context;

/* oka::Scene::Vertex (include/scene/scene.h:80-89) == Vertex (OptixRenderParams.h:19-28): 32 B AoS.
 * normal/tangent: 10-10-10 packed (scene.cpp:111-117), uv: 16-16 packed over [-10,10] (RenderPass.cpp:53-67). */
typedef struct skh_vertex
{
    float pos[3];
    uint32_t tangent;
    uint32_t normal;
    uint32_t uv;
    float pad0;
    float pad1;
} skh_vertex;

/* oka::Mesh (include/scene/scene.h:21-27).  Indices are mesh-local; vertex_offset is added at fetch time
 * (OptixRender_radiance_closest_hit.cpp:365-376). */
typedef struct skh_mesh
{
    uint32_t index_offset; /* mIndex    */
    uint32_t index_count;  /* mCount    */
    uint32_t vertex_offset; /* mVbOffset */
    uint32_t vertex_count; /* mVertexCount */
} skh_mesh;

/* oka::Curve (include/scene/scene.h:29-42); always cubic B-spline on the render side
 * (OptixRender.cpp:218-245: degree 3, segments = n-3 per strand). */
typedef struct skh_curve
{
    uint32_t vertex_counts_start;
    uint32_t vertex_counts_count;
    uint32_t points_start;
    uint32_t points_count;
    uint32_t widths_start;
    uint32_t widths_count;
} skh_curve;

/* oka::Instance::Type (include/scene/scene.h:47-52) */
enum
{
    SKH_INSTANCE_MESH = 0,
    SKH_INSTANCE_LIGHT = 1,
    SKH_INSTANCE_CURVE = 2
};

/* oka::Instance (include/scene/scene.h:44-60) with the transform already in the 3x4 row-major
 * object-to-world form the reference hands to OptiX (OptixRender.cpp:438). 64 B. */
typedef struct skh_instance
{
    float transform[12]; /* row-major 3x4, object -> world */
    uint32_t type; /* SKH_INSTANCE_* */
    uint32_t geom_id; /* mMeshId / mCurveId */
    uint32_t material_id; /* 0xffffffff -> material 0 (OptixRender.cpp:768) */
    uint32_t light_id; /* only for SKH_INSTANCE_LIGHT */
} skh_instance;

/* oka::Scene::Light == UniformLight (include/render/Lights.h:5-14): 112 B.
 * type: 0 rect, 1 disc (no sampler/pdf in the reference), 2 sphere, 3 distant. */
typedef struct skh_light
{
    float points[4][4];
    float color[4];
    float normal[4];
    int32_t type;
    float half_angle;
    float pad0;
    float pad1;
} skh_light;

/* Fixed-layout "MDL-equivalent" material argument block (replaces the MDL SDK generated argument
 * block + PTX: OptixRender.cpp:1270-1433, materialmanager.cpp:524-609).  64 B. */
enum
{
    SKH_MAT_DIFFUSE = 0, /* default.mdl::default_material(diffuse_color)  (OptixRender.cpp:1090-1097) */
    SKH_MAT_PBR = 1, /* OmniPBR: diffuse_color_constant, reflection_roughness_constant, metallic_constant */
    SKH_MAT_GLASS = 2, /* OmniGlass: glass_color, glass_ior, frosting_roughness (thin_walled = false; gltfloader.cpp:354-406) */
    SKH_MAT_HAIR = 3 /* hair sub-expression (mdlPtxCodeGen.cpp:143-155): df::chiang_hair_bsdf */
};

/* Field use per type:
 *   DIFFUSE  base_color = diffuse_color
 *   PBR      base_color = diffuse_color_constant, roughness = reflection_roughness_constant, metallic = metallic_constant,
 *            specular = specular_level
 *   GLASS    base_color = glass_color, ior = glass_ior, roughness = frosting_roughness (< 1e-3: clear glass, specular events;
 *            else a rough dielectric, Walter et al. 2007 / GGX with alpha = roughness^2, glossy events)
 *   HAIR     the arguments of df::chiang_hair_bsdf (Chiang et al. 2016): base_color = diffuse_reflection_tint,
 *            roughness = roughness_R.x, metallic = roughness_TT.x and specular = roughness_TRT.x (<= 0: derived from R as in the
 *            paper, v_TT = v_R / 4, v_TRT = 4 v_R), ior = ior, reserved[0..2] = absorption_coefficient, reserved[3] = azimuthal
 *            roughness (roughness_*.y), reserved[4] = cuticle_angle (radians), reserved[5] = diffuse_reflection_weight */
typedef struct skh_material
{
    uint32_t type; /* SKH_MAT_* */
    float base_color[3];
    float roughness;
    float metallic;
    float specular; /* specular_level, OmniPBR default 0.5 */
    float ior;
    /* Texture ids (1-based index into skh_set_textures' list, 0 = none -- MDL numbers its resources from 1, 0 being the
     * invalid texture: texture_support_cuda.h:300-304).  OmniPBR "diffuse_texture" / "normalmap_texture"
     * (gltfloader.cpp:336-350): a valid diffuse texture replaces base_color, a valid normal map perturbs state.normal.
     * Roughness, metallic and emission maps travel beside this record: skh_set_material_textures. */
    uint32_t base_color_texture;
    uint32_t normal_texture;
    float reserved[6];
} skh_material;

/* One 2-D texture as the reference loads it: stbi_load(..., STBI_rgb_alpha) -> uchar4 array, sampled with
 * cudaReadModeNormalizedFloat / cudaFilterModeLinear / cudaAddressModeWrap / normalized coordinates
 * (OptixRender.cpp:1191-1264; lookup: texture_support_cuda.h:287-313).  Row 0 first, 4 bytes per texel. */
typedef struct skh_texture
{
    const uint8_t* rgba8;
    uint32_t width, height;
} skh_texture;

/* Per-launch constants == the subset of Params (OptixRenderParams.h:38-68) that render() fills
 * every call (OptixRender.cpp:936-1004). Matrices are ROW-major (OptixRender.cpp:953-954). */
typedef struct skh_frame_params
{
    float view_to_world[16];
    float clip_to_view[16];
    uint32_t subframe_index; /* Params::subframe_index      */
    uint32_t samples_this_launch; /* Params::samples_per_launch  */
    uint32_t spp_total; /* Params::maxSampleCount      */
    uint32_t max_depth; /* Params::max_depth           */
    uint32_t rect_light_sampling_method; /* 0 uniform, 1 spherical rectangle */
    float exposure[3];
    uint32_t enable_accumulation;
    uint32_t debug; /* 0 none, 1 normals, 2 diffuse AOV, 3 specular AOV */
    float shadow_ray_tmin;
    float material_ray_tmin;
} skh_frame_params;

/* One ray for skh_trace (the optixTrace call sites: OptixRender.cu:120-129, closest_hit.cu:185-197). */
typedef struct skh_ray
{
    float origin[3];
    float tmin;
    float dir[3];
    float tmax;
} skh_ray;

/* What optixGetRayTmax / optixGetInstanceIndex / optixGetPrimitiveIndex /
 * optixGetTriangleBarycentrics / optixGetCurveParameter return.  20 B. */
typedef struct skh_hit
{
    float t; /* < 0 : miss */
    uint32_t instance_id; /* 0xffffffff : miss */
    uint32_t prim_id;
    float u; /* triangle barycentric u, or curve parameter */
    float v;
} skh_hit;

enum
{
    SKH_TRACE_CLOSEST = 0, /* visibility mask 255 (OptixRender.cu:124) */
    SKH_TRACE_SHADOW = 1 /* RAY_MASK_SHADOW, terminate on first hit; hit.t = 1 if occluded, -1 if not */
};

enum
{
    /* Which builder skh_build_accel runs (all on the GPU; hit records do not depend on the choice).  The NAMES are north_star's ("LBVH / SAH refit");
     * what they select:
     *   SKH_BUILD_LBVH (0)  the context's default = option "build_quality": 1 (default) -> the same builder as SKH_BUILD_SAH below;
     *                       0 -> a plain Karras 2012 radix tree over the Morton order (fastest build, ~25 % more node visits per ray).
     *   SKH_BUILD_SAH  (1)  the quality builder, whatever the option says: Morton sort -> PLOC agglomerative clustering (Meister & Bittner 2018a) ->
     *                       rounds of parallel reinsertion (Meister & Bittner 2018b; the sum of the internal boxes' areas is the cost it lowers) ->
     *                       collapse to 4-wide quantised nodes.  "SAH-class": it minimises a surface-area cost, it is not a sweep / binned SAH.
     * REFIT: skh_refit_accel below (topology kept, leaf records and boxes recomputed: kitchen stand-in 2.2 ms against 61 ms for the build) -- the
     * reference builds its acceleration structures once, on frame 0, and ignores later edits (OptixRender.cpp:876). */
    SKH_BUILD_LBVH = 0,
    SKH_BUILD_SAH = 1
};

typedef struct skh_stats
{
    uint64_t rays_radiance; /* closest-hit rays traced since the last reset for sub-frames that were DELIVERED (see speculated_discarded) */
    uint64_t rays_shadow; /* any-hit rays, likewise */
    /* traversal counters, counter build only (skh_set_option "count_traversal"); [0] closest-hit kernel,
     * [1] shadow (any-hit) kernel */
    uint64_t nodes_visited[2]; /* 64-byte BVH nodes fetched */
    uint64_t prims_tested[2]; /* triangles */
    uint64_t segs_tested[2]; /* curve segments */
    uint64_t instances_entered[2];
    double ms_trace_closest; /* hipEvent time summed over launches since the last reset */
    double ms_trace_shadow;
    double ms_shade;
    double ms_raygen;
    double ms_accumulate;
    double ms_build; /* last skh_build_accel */
    double ms_sort; /* always 0 (ray re-ordering, a measured negative of round 1, was removed in round 3) */
    uint32_t launches_trace_closest;
    uint32_t launches_trace_shadow;
    uint32_t launches_shade;
    uint32_t launches_other;
    /* render / trace calls since the last reset that returned SKH_FAIL because a traversal stack (20 LDS + 104 global entries per
     * ray) overflowed and dropped a subtree -- a degenerate hierarchy; such a call's hits may be incomplete */
    uint32_t stack_overflows;
    /* sub-frames skh_render_subframe traced ahead (option speculate) and had to throw away since the last reset -- the caller moved
     * the camera, changed the scene or resized; their rays are NOT in rays_radiance / rays_shadow */
    uint32_t speculated_discarded;
} skh_stats;

/* ---- lifetime: RenderFactory::createRender + Render::init (render.cpp:10-35, OptixRender.cpp:1059-1105) ---- */
skh_status skh_create(int device_ordinal, skh_context** out_ctx);
void skh_destroy(skh_context* ctx);
const char* skh_last_error(const skh_context* ctx);
uint32_t skh_abi_version(void);

/* ---- scene upload: createVertexBuffer/IndexBuffer/PointsBuffer/WidthsBuffer/LightBuffer
 *      (OptixRender.cpp:1117-1189), reading oka::Scene getters (scene.h:229-327) ---- */
skh_status skh_set_geometry(skh_context* ctx, const skh_vertex* verts, uint32_t n_verts, const uint32_t* indices,
                            uint32_t n_indices, const skh_mesh* meshes, uint32_t n_meshes);
skh_status skh_set_curves(skh_context* ctx, const float* points_xyz, uint32_t n_points, const float* radii,
                          uint32_t n_radii, const uint32_t* vertex_counts, uint32_t n_vertex_counts,
                          const skh_curve* curves, uint32_t n_curves);
skh_status skh_set_instances(skh_context* ctx, const skh_instance* instances, uint32_t n_instances);
skh_status skh_set_lights(skh_context* ctx, const skh_light* lights, uint32_t n_lights);
/* Replaces the texture list (count may be 0).  Host pointers need only live for the call. */
skh_status skh_set_textures(skh_context* ctx, const skh_texture* textures, uint32_t count);
skh_status skh_set_materials(skh_context* ctx, const skh_material* materials, uint32_t n_materials);

/* ---- environment (dome) light: new, the reference declares HdPrimTypeTokens->domeLight (src/HdStrelka/RenderPass.cpp:383) and never creates one ----
 * A lat-long map of linear float RGB that every ray leaving the scene sees, importance-sampled by the light pick ("Environment light").
 *   map        row 0 = the +Y pole, column 0 at phi = 0 on +X, phi growing towards +Z; 2 <= width <= 8192, 2 <= height <= 4096; finite values >= 0
 *   look-up    l = world_to_env * d, theta = acos(clamp(l.y)), phi = atan2(l.z, l.x) (+ 2 pi if negative);
 *              ix = min(int(phi / 2 pi * W), W - 1), iy = min(int(theta / pi * H), H - 1); nearest texel; Le = scale * texel
 *   sampling   texel weight w = luminance_709(texel) * sin(pi (iy + 1/2) / H); marginal CDF over rows, conditional CDF per row, CDF inversion, uniform inside the
 *              texel; pdf per solid angle of a direction = w / sum w * W H / (2 pi^2 sin theta), sin theta = sqrt(l.x^2 + l.z^2); an all-black map is legal (pdf 0)
 *   light pick with an environment the pick has numLights + 1 entries, the last one being the environment (selection pdf 1 / (numLights + 1)); a ray that
 *              misses adds throughput * Le * weight, weight = 1 at depth 0 or after a specular bounce, else the balance heuristic of the BSDF's pdf against
 *              pdf / (numLights + 1).  Option env_nee 0: never picked, every miss weighs 1.
 * skh_set_environment uploads the map and builds the tables on the device (rgb == NULL removes the environment: the context then runs the kernels and produces
 * the bits of one that never had any).  skh_set_environment_transform changes scale / rotation only -- no rebuild -- and needs an environment.  Both discard
 * sub-frames traced ahead, as skh_set_lights does; neither touches the acceleration structures.  A failed call leaves the previous environment in place. */
typedef struct skh_environment
{
    const float* rgb; /* width * height * 3; NULL = remove the environment */
    uint32_t width, height;
    float scale[3]; /* intensity * colour */
    float world_to_env[9]; /* row-major rotation */
} skh_environment;
skh_status skh_set_environment(skh_context* ctx, const skh_environment* env);
skh_status skh_set_environment_transform(skh_context* ctx, const float scale[3], const float world_to_env[9]);
typedef struct skh_environment_info
{
    uint32_t width, height; /* 0, 0: no environment */
    double sum_w; /* sum of the texel weights */
    double ms_build; /* wall time of the table build (device kernels, without the upload of the map) */
    uint64_t bytes; /* device memory of the tables: 16 B texels + 4 B conditional CDF per texel + the marginal CDF */
} skh_environment_info;
skh_status skh_get_environment_info(skh_context* ctx, skh_environment_info* out);

/* ---- emissive meshes: new, the reference generates mdl_edf_emission_* for every material (src/materialmanager/mdlPtxCodeGen.cpp:14-15,140-159) and no hit program calls them ----
 * One linear RGB radiance Le per material, indexed as the material list is ("Emissive meshes").  Hits on mesh instances only; a triangle emits from
 * its front side, the one its world-space geometric normal points to, and still reflects.
 *   emitter table  one entry per (mesh instance whose material emits, triangle of its mesh), world space, built on the device: weight w_k = world area * luminance_709(Le),
 *                  sum w in double, an inclusive CDF of floats (each one rounding away from the exact CDF of the stored weights) and a guide table over it.
 *                  64 B per entry (three world-space vertices, Le, ids) + 4 B CDF + at most 8 B guide; at most SKH_EMIT_MAX_ENTRIES = 2^24 entries -- a scene
 *                  with more is refused with SKH_INVALID_ARGUMENT by the call that builds the table (render, probe, info)
 *   light pick     the whole emitter set is ONE more entry of the pick, behind the lights and the environment; the triangle by CDF inversion of the fraction of the pick's own
 *                  draw, the point uniform on it; pdf per solid angle = luminance_709(Le) / sum w * dist^2 / cos at the emitter; no second surface cosine (as the environment)
 *   hit            radiance += throughput * Le * weight, weight = 1 at depth 0, after a specular bounce or with option emit_nee 0, else the balance heuristic of the
 *                  BSDF's pdf against pdf / entries of the pick
 * skh_set_emission: rgb = 3 * n_materials floats, finite and >= 0, n_materials <= the material count; materials beyond n do not emit.  NULL or 0 removes all emission: the
 * context then runs the kernels and produces the bits of one that never had any.  Discards sub-frames traced ahead, as skh_set_lights does; never touches the acceleration
 * structures; a failed call leaves the previous emission in place.  The table is derived data: stale after skh_set_geometry / _instances / _materials / _emission and after
 * skh_update_accel with a new instance table, rebuilt on the device before the next render, probe or info call; it needs no acceleration structure. */
#define SKH_EMIT_MAX_ENTRIES (1u << 24)
skh_status skh_set_emission(skh_context* ctx, const float* rgb, uint32_t n_materials);
typedef struct skh_emitter_info
{
    uint32_t triangles, instances; /* entries of the table and the mesh instances they come from; 0, 0: nothing emits */
    double sum_w; /* sum of the entry weights */
    double ms_build; /* wall time of the last table build (device kernels and the small uploads) */
    uint64_t bytes; /* device memory of the table */
} skh_emitter_info;
skh_status skh_get_emitter_info(skh_context* ctx, skh_emitter_info* out);
/* The device functions k_shade calls, on host arrays of packed 32-bit words (n records):
 *   SKH_EMIT_PROBE_SAMPLE  in  f32 u' (the selection draw), ux, uy, P[3] (the shaded point)
 *                          out f32 point[3], normal[3], Le[3], pdf per solid angle (without the pick's 1 / entries), dist, u32 instance, prim
 *                          (Le at the sampled point: times the emission map's texel when skh_set_material_textures bound one; this kind then needs the build's shading records)
 *   SKH_EMIT_PROBE_PDF     in  u32 instance, prim, f32 hitPoint[3], origin[3]      out f32 pdf, Le[3]   (0s for a triangle that is not in the table) */
#define SKH_EMIT_PROBE_SAMPLE 0u
#define SKH_EMIT_PROBE_PDF 1u
skh_status skh_emitter_probe(skh_context* ctx, uint32_t kind, const void* in, uint32_t n, void* out);

/* ---- Material textures: roughness, metallic / ORM and emission maps (DESIGN.md section 2 "Material textures") ----
 * What OmniPBR's reflectionroughness_texture, metallic_texture, ORM_texture, emissive_color_texture and emissive_mask_texture and glTF's metallicRoughnessTexture and
 * emissiveTexture do, as one table beside the material list.  The look-up is base colour's: bilinear, wrap, 1.8 fixed-point weights, the raw 8-bit values / 255 with
 * no sRGB decode, at the hit's interpolated text_coords[0]; triangle hits only.
 *   roughness, metallic   SKH_MAT_PBR materials: value = clamp01(scale * texel + bias), the product and the sum rounded separately (no fma).  OmniPBR's
 *                         mix(constant, texel, influence): scale = influence, bias = constant * (1 - influence); glTF's factor * texel: scale = factor, bias = 0.
 *                         Two slots that name the same texture id share ONE look-up (ORM: roughness = g, metallic = b).
 *   emission              every material skh_set_emission gave an Le: Le(x) = Le_material * texel (rgb, or one channel for all three), at an emitter hit and at an
 *                         emitter sample (the uv there from the triangle's vertices at the sample's barycentrics).  The emitter table keeps its material-level weights
 *                         area * luminance(Le_material) and the pdfs do not change: the estimator stays unbiased, a dark part of a map only wastes picks.  A material
 *                         whose Le is 0 does not emit, whatever its map.
 * One entry per material, indexed as the material list; 48 B.  Texture ids as skh_material's: 1-based into skh_set_textures' list, 0 = none, an id beyond the list = none. */
typedef struct skh_material_textures
{
    uint32_t roughness_texture, metallic_texture, emission_texture;
    uint32_t roughness_channel, metallic_channel; /* 0..3 = r, g, b, a */
    uint32_t emission_channel; /* 0..3 = that channel for all three, 4 = rgb */
    float roughness_scale, roughness_bias; /* roughness = clamp01(scale * texel + bias) */
    float metallic_scale, metallic_bias;
    uint32_t reserved[2]; /* must be 0 */
} skh_material_textures;
/* n_materials <= the material count; materials beyond n bind nothing.  NULL or 0 removes the table: the context then runs the kernels and produces the bits of one that
 * never had any -- as does a table in which no entry binds a texture that exists.  A channel out of range, a scale or bias that is not finite or a non-zero reserved word
 * is refused with SKH_INVALID_ARGUMENT and leaves the previous table in place.  Discards sub-frames traced ahead; never touches the acceleration structures or the
 * emitter table. */
skh_status skh_set_material_textures(skh_context* ctx, const skh_material_textures* entries, uint32_t n_materials);
/* The device function k_shade calls for a triangle hit of `material[i]` at uv[2 i], uv[2 i + 1]: out[8 i ...] = base_color[3], roughness, metallic, Le[3] (all of it
 * after the textures; a context without a table answers with base_color_texture alone). */
skh_status skh_material_probe(skh_context* ctx, uint32_t n, const uint32_t* material, const float* uv, float* out);

/* ---- Cutouts: opacity maps tested between trace and shade (DESIGN.md section 2 "Cutouts") ----
 * What glTF's alphaMode MASK / alphaCutoff, OmniPBR's enable_opacity / opacity_texture / opacity_threshold and UsdPreviewSurface's opacityThreshold do: a hit whose
 * opacity is below the threshold is no hit, for radiance rays and for shadow rays.  It changes which hit a ray has, so it sits at the traversal level -- not inside the
 * trace kernels: a stage of its own (k_cutout) looks at the hit records of a trace launch and re-queues the rays whose hit is cut away.
 * One entry per material, indexed as the material list is; 32 B.
 *   look-up       tex_lookup_rgba8, unchanged: bilinear, wrap, 1.8 fixed-point weights, raw 8-bit value / 255; at the hit's interpolated text_coords[0], computed as
 *                 k_shade computes it for the base colour.  Hits on mesh instances only (SKH_INSTANCE_MESH): curve instances and light proxies are never cut.
 *   closest hit   a ray's hit is the nearest ACCEPTED one.  When the hit at t is rejected the ray goes on with the same origin, the same direction, tmin = t and the
 *                 same tmax.  The intersectors accept tmin < t' <= tmax, so the rejected primitive cannot come back -- and neither can anything else at exactly that
 *                 t: a second surface at bit-exactly the rejected distance is skipped with it (part of the definition).  Path depth, sampler dimensions, lastBsdfPdf,
 *                 the MIS distance of an emitter hit and the offset_ray of the next bounce are those of the ray that produced the accepted hit from the start: an
 *                 image with a cut-away triangle equals, bit for bit, the image of the scene without that triangle.
 *   shadow rays   occluded iff an accepted hit lies in (tmin, tmax].  Hits on instances the shadow mask excludes (light proxies, baked hidden ones too) pass through.
 *   round limit   option cutout_rounds (default 8, 1..32): the number of rejected hits per ray.  After that many the next hit is accepted whatever its opacity (for a
 *                 shadow ray it occludes; a light proxy met there still does not).  Deterministic, no host round trip.  A light proxy a shadow ray passes through
 *                 uses up a round like a rejected hit.
 *   emission      a material that both emits (skh_set_emission gave it an Le != 0) and has an active cutout is refused with SKH_INVALID_ARGUMENT, the message naming
 *                 the material, by the call that would use it: render, trace or info.
 * Not part of it: cutouts on curves, coloured transmission, an alpha test inside the traversal loop.  (Fractional opacity -- threshold 0 with opacity < 1, glTF BLEND --
 * is a table of its own: skh_set_material_blend, below.) */
typedef struct skh_material_cutout
{
    uint32_t opacity_texture;   /* 1-based into skh_set_textures' list; 0 or beyond the list = no texture: texel = 1 */
    uint32_t opacity_channel;   /* 0..3 = r, g, b, a */
    float opacity_scale, opacity_bias; /* opacity = clamp01(scale * texel + bias), product and sum rounded separately */
    float threshold;            /* 0 = entry inactive (opaque); else in (0, 1]: the hit counts iff opacity >= threshold */
    uint32_t reserved[3];       /* must be 0 */
} skh_material_cutout;
/* n_materials <= the material count; materials beyond n are opaque.  NULL or 0 removes the table; a table in which no entry is active, or whose active materials no mesh
 * instance uses, equals no table: the context then launches the kernels (the any-hit shadow kernel among them) and produces the bits of one that never had any.  A channel
 * above 3, a scale or bias that is not finite, a threshold outside [0, 1] or a non-zero reserved word is refused with SKH_INVALID_ARGUMENT and leaves the previous table in
 * place.  Discards sub-frames traced ahead; never touches the acceleration structures or the emitter table.  Whether a cutout is in use is derived data: recomputed after
 * skh_set_materials / _textures / _instances / _material_cutouts / _emission and after skh_update_accel with a new instance table.  skh_trace and skh_trace_device honour
 * the table in both modes. */
skh_status skh_set_material_cutouts(skh_context* ctx, const skh_material_cutout* entries, uint32_t n_materials);
typedef struct skh_cutout_info
{
    uint32_t active_materials; /* entries with threshold > 0 (inside the material list) */
    uint32_t instances; /* mesh instances that use one of them; 0: the cutout stage does not run */
    uint64_t continued_closest, continued_shadow; /* rays re-queued because their hit was cut away, since the last skh_reset_stats (not part of rays_radiance / rays_shadow) */
    uint64_t accepted_by_cap; /* hits that are cut away and were accepted by the round limit */
    uint64_t bytes; /* device memory of the continuation queues and the extra hit buffers */
} skh_cutout_info;
skh_status skh_get_cutout_info(skh_context* ctx, skh_cutout_info* out);

/* ---- Fractional opacity: stochastic pass-through for radiance rays, transmittance for shadow rays (DESIGN.md section 2 "Fractional opacity") ----
 * What glTF's alphaMode BLEND, OmniPBR's enable_opacity without a threshold and UsdPreviewSurface's opacity < 1 without an opacityThreshold ask for: smoke cards, decals,
 * soft-edged leaf and hair cards, gauze.  Not refraction: the ray goes straight on.  The same stage as the cutouts (k_cutout, its BLEND build), the same continuation
 * rounds, the same round limit; one entry per material, indexed as the material list is; 32 B.
 *   opacity       a = clamp01(scale * texel + bias), product and sum rounded separately; the texel as the cutouts look it up (tex_lookup_rgba8 at the hit's interpolated
 *                 text_coords[0]); no texture: texel = 1.  Hits on mesh instances only (SKH_INSTANCE_MESH): curves and light proxies are never blended.
 *   radiance rays take the hit iff xi < a (a = 1 always, a = 0 never).  A ray that does not goes on as a cut-away ray does: same origin and direction, tmin = t, same
 *                 tmax, its queue position kept; depth, sampler dimensions, lastBsdfPdf, the MIS distance of an emitter hit and the next bounce's offset_ray are
 *                 those of the ray that produced the accepted hit.  An accepted hit is shaded at full weight (no factor a): E = a * shade + (1 - a) * behind.
 *   the draw      xi = (h >> 8) * 2^-24, h = hash_murmur(hash_combine(hash_combine(hash_murmur(sampleIdx ^ 0xb5297a4d), depth), round)); sampleIdx is the sampler's
 *                 (encode_morton2(px, py) * spp_total + pixel sample index), depth the bounce whose trace launch produced the record, round the number of hits this
 *                 ray has already passed.  A pure function of the path and the ray's progress: it does not depend on scheduling, sub-frame batching, speculation or
 *                 tile ownership.  White noise, not a Sobol dimension.  (strelka_amd/csrc/skh_blend.h, which a host program compiles too; skh_blend_probe evaluates it on the device.)
 *   shadow rays   attenuated, not gambled: occluded iff an opaque hit lies in (tmin, tmax] -- a material without a blend entry, a blend hit with a >= 1, a cutout that
 *                 accepts.  Otherwise the light sample's contribution is multiplied, per blend hit crossed and in order of increasing t, by w = 1 - a: one rounded
 *                 subtraction, one rounded product per channel.  a = 0 leaves its bits unchanged.
 *   round limit   cutout_rounds, shared with the cutouts: every passed hit -- cut away, blended, or a light proxy in a shadow ray's way -- uses up a round.  After that
 *                 many the next hit is accepted whatever its opacity, and a shadow ray is occluded by it (a light proxy still does not occlude).
 *   raw queries   skh_trace / skh_trace_device have no sample: a blend hit counts iff a > 0, in both modes.
 *   refused       with SKH_INVALID_ARGUMENT, the message naming the material, by the call that would use it (render, trace, info): a material with both an active
 *                 cutout and an active blend entry; a material that emits and has an active blend entry.
 * Not part of it: coloured transmission, blending on curves, stratified draws. */
typedef struct skh_material_blend
{
    uint32_t opacity_texture;   /* 1-based into skh_set_textures' list; 0 or beyond the list = no texture: texel = 1 */
    uint32_t opacity_channel;   /* 0..3 = r, g, b, a */
    float opacity_scale, opacity_bias; /* a = clamp01(scale * texel + bias), product and sum rounded separately */
    uint32_t active;            /* 0 = opaque (the entry is ignored), 1 = blended */
    uint32_t reserved[3];       /* must be 0 */
} skh_material_blend;
/* n_materials <= the material count; materials beyond n are opaque.  NULL or 0 removes the table; a table in which no entry is active, or whose active materials no mesh
 * instance uses, equals no table: the context launches the kernels and produces the bits of one that never had any (with threshold cutouts alone in use: the stage of
 * before, k_cutout's build without BLEND).  A channel above 3, a scale or bias that is not finite, active > 1 or a non-zero reserved word is refused with
 * SKH_INVALID_ARGUMENT and leaves the previous table in place.  Discards sub-frames traced ahead; never touches the acceleration structures or the emitter table.
 * Whether blending is in use is derived data, recomputed after the calls that make the cutouts' stale. */
skh_status skh_set_material_blend(skh_context* ctx, const skh_material_blend* entries, uint32_t n_materials);
typedef struct skh_blend_info
{
    uint32_t active_materials; /* entries with active = 1 (inside the material list) */
    uint32_t instances; /* mesh instances that use one of them; 0: blending is not in use */
    uint64_t passed_radiance; /* radiance rays that went on through a blend hit (xi >= a), since the last skh_reset_stats */
    uint64_t crossed_shadow; /* blend hits shadow rays crossed (each scaled the contribution by 1 - a) */
    uint64_t accepted_by_cap; /* blend hits the draw (or, for a shadow ray, a < 1) would have passed and the round limit accepted */
    uint64_t bytes; /* device memory of the stage's buffers: the continuation queues and extra hit buffers it shares with the cutouts (skh_cutout_info.bytes counts the same ones) */
} skh_blend_info;
skh_status skh_get_blend_info(skh_context* ctx, skh_blend_info* out);
/* The draw, evaluated on the device by the function k_cutout calls: in = n x {px, py, pixel sample index, spp_total, depth, round}, xi = n floats in [0, 1). */
skh_status skh_blend_probe(skh_context* ctx, uint32_t n, const uint32_t* in, float* xi);

/* ---- Light shapes: sampled disk lights and UsdLux shaping cones (DESIGN.md section 2 "Light shapes") ----
 * Two things the reference's analytic lights cannot do.  A disk light (type 1) has a proxy and neither a sampler nor a pdf (Lights.h): it shines only where a BSDF-sampled
 * ray happens to hit its proxy, and wastes its share of the light pick.  And no light can be narrowed: UsdLux ShapingAPI (shaping:cone:angle, shaping:cone:softness,
 * shaping:focus) is how every spot lamp is authored.  One entry per light, indexed as the light list is; 32 B.
 *   SAMPLE_DISC   (type 1) the light takes part in next-event estimation.  The light is what rays can hit -- the 16-gon of the proxy, not the analytic disc: with
 *                 O = points[1], X = points[2].xyz, Y = points[3].xyz the vertices v_k = O + cos(2 pi k / 16) X + sin(2 pi k / 16) Y, the area A = 8 sin(pi / 8) |X x Y|,
 *                 the unit normal n = normalize(light.normal) (the reference stores it scaled by the radius; the flagged disk uses it normalised, in the sampler and at
 *                 the hit).  A draw (ux, uy): sector k = min(int(16 ux), 15), u' = 16 ux - k (exact), a uniform point of the triangle (O, v_k, v_k+1) from (u', uy) by the
 *                 emitter table's mapping.  Everything else is the rect light's protocol: pdf = dist^2 / (dot(-L, n) A), the two front-side tests,
 *                 lrad = Li saturate(dot(N, L)), the pick's 1 / entries.  At a proxy hit the radiance term uses -dot(rayD, n) with the unit normal and the MIS weight
 *                 the same pdf / entries of the pick.  A disk without the flag is what it was, bit for bit.
 *   CONE          (types 0, 1, 2) emission scaled by s(c), c = dot(axis, w), w the unit direction from the light point to the shaded point (-L at a light sample,
 *                 -rayD at a proxy hit -- at depth 0 and after a specular bounce too): s = 0 unless c > cos_outer; else t = min((c - cos_outer) / (cos_inner - cos_outer), 1)
 *                 (1 for a hard edge), s = t^2 (3 - 2 t) * (focus > 0 ? pow(max(c, 0), focus) : 1).  Pdfs and the pick do not change: the estimator stays unbiased, a
 *                 dark direction only wastes a pick (and queues no shadow ray).
 * Not part of it: cylinder lights, IES profiles, focusTint, solid-angle sampling of sphere lights, cones on distant lights, the environment or emissive meshes. */
#define SKH_LIGHT_SHAPE_SAMPLE_DISC 1u /* type 1 only: the light takes part in next-event estimation */
#define SKH_LIGHT_SHAPE_CONE 2u /* types 0, 1, 2: emission scaled by s(c) */
typedef struct skh_light_shape
{
    uint32_t flags;
    float cos_outer;   /* cos(shaping:cone:angle) */
    float cos_inner;   /* cos(angle * (1 - softness)) >= cos_outer; equal = hard edge */
    float focus;       /* shaping:focus, >= 0; 0 = none */
    float axis[3];     /* unit, world space: the direction the light shines along */
    uint32_t reserved; /* must be 0 */
} skh_light_shape;
/* n_lights <= the light count; lights beyond n are plain.  NULL or 0 removes the table; a table in which no entry has a flag that applies to its light's type (SAMPLE_DISC:
 * type 1; CONE: types 0, 1, 2; both ignored elsewhere) equals no table: the context launches the kernels and produces the bits of one that never had any.  Flags above 3,
 * a cosine outside [-1, 1] or not finite, cos_inner < cos_outer, a focus that is negative or not finite, with CONE set an axis that is not finite or whose length is off 1
 * by more than 1e-3, or a non-zero reserved word is refused with SKH_INVALID_ARGUMENT and leaves the previous table in place.  Discards sub-frames traced ahead; never
 * touches the acceleration structures or the emitter table.  Which entries are in use is derived data, recomputed after skh_set_lights and skh_set_light_shapes. */
skh_status skh_set_light_shapes(skh_context* ctx, const skh_light_shape* entries, uint32_t n_lights);
typedef struct skh_light_shape_info
{
    uint32_t sampled_discs; /* entries in use inside the light list: SAMPLE_DISC on a type-1 light */
    uint32_t cones; /* CONE on a light of type 0, 1 or 2; both 0: the kernels of a context without a table run */
} skh_light_shape_info;
skh_status skh_get_light_shape_info(skh_context* ctx, skh_light_shape_info* out);
/* The device functions k_shade calls, on host arrays of packed 32-bit words (n records), against the context's light list and shape table:
 *   SKH_LSHAPE_PROBE_SAMPLE  in  u32 light, f32 ux, uy, P[3] (the shaded point)
 *                            out f32 point[3], normal[3], L[3], dist, pdf per solid angle (without the pick's factor), s, area
 *   SKH_LSHAPE_PROBE_PDF     in  u32 light, f32 lightHitPoint[3], surfacePoint[3]      out f32 pdf, s
 * Lights of types 0, 2 and 3 answer with the existing samplers' values (a rect light by the uniform method), s applied when a cone is set (else 1); a disk without
 * SAMPLE_DISC with the zero sample it always was; a light index beyond the list with zeros. */
#define SKH_LSHAPE_PROBE_SAMPLE 0u
#define SKH_LSHAPE_PROBE_PDF 1u
skh_status skh_light_shape_probe(skh_context* ctx, uint32_t kind, const void* in, uint32_t n, void* out);

/* ---- createAccelerationStructure (OptixRender.cpp:388-496): per-mesh / per-curve BLAS + one TLAS ---- */
skh_status skh_build_accel(skh_context* ctx, uint32_t flags);
/* After a VERTEX edit -- skh_set_geometry with the mesh table and index buffer of the last build, any vertex data; skh_set_curves with the curve sets and vertex
 * counts of the last build, any control points and radii (an animated groom) -- keep the hierarchies' topology and
 * recompute its leaf records and boxes bottom-up (north_star's "SAH refit"; the reference has no equivalent: it builds once, on frame 0, OptixRender.cpp:876).
 * Refits when every mesh instance is baked to world space (no top level: what a bake without mesh sharing gives) and nothing but the vertices changed since
 * the build; otherwise it IS skh_build_accel(flags of the last build).  skh_build_info.refit says which happened.  Hit records do not depend on the hierarchy,
 * so a refitted tree returns what a rebuilt one returns; after large deformations a rebuild traverses faster.  Kitchen stand-in (23 M world-space triangles,
 * 6.06 M nodes): build 61 ms, refit 2.2 ms. */
skh_status skh_refit_accel(skh_context* ctx);
/* After edits that keep every hierarchy's topology -- instance TRANSFORMS, vertices (skh_set_geometry with the built mesh table and index buffer), curve control
 * points and radii (skh_set_curves with the built curve sets and vertex counts), in any combination, for every scene kind -- update every level of the
 * acceleration structure in place: the triangle and curve trees (the baked world-space triangles carry their instances' transforms) are refitted when their
 * primitives moved, the instance records and world boxes recomputed, the TLAS keeps its tree and leaf order and is refitted level by level on the GPU.  The
 * reference has the edit channel (Scene::updateInstanceTransform / getDirtyInstances, include/scene/scene.h:437-455) and never reads it.
 *   instances  the instance table of the last build (or update) with any TRANSFORMS -- type, geom_id, material_id, light_id unchanged -- and n_instances its
 *              count; NULL (n_instances 0) = the table as it is (skh_set_instances may have set it).
 * skh_build_info.refit = 2 and ms_refit = the wall time when it updated in place.  Otherwise it IS skh_set_instances(instances) + skh_build_accel(flags of the
 * last build), refit = 0, results as exact; that happens for
 *   - no build yet, or an option changed since the last one (every option that changes a hierarchy clears it);
 *   - another instance count, or an instance whose type, geom_id, material_id or light_id changed (what the bake and the TLAS leaves are made of);
 *   - another mesh table / index buffer, or other curve sets / vertex counts (topology: the refit's own rule);
 *   - a transform that became singular (invert_affine fails) or stopped being singular: the instance gains or loses its TLAS leaf and its bake;
 *   - a world-curve entry (a curve tree the world-only kernel enters itself) whose transform left or reached the bit-exact identity: the build orders the
 *     table by it and lets the kernel skip the identity's matrix (SKH_REF_CURVEROOT_IDENT);
 *   - members of a merged curve group (option curve_merge) that no longer share one transform: their segments sit in ONE tree, in the group's object space;
 *   - tlas_open > 1 (experimental): the opened TLAS leaves are BLAS subtrees whose boxes the build made from the transforms;
 *   - the experimental segment-node curve build (curve_segnode), which has no refit.
 * Hit records do not depend on the hierarchy, so the updated structure returns what a rebuild returns; the trees keep the shape they were built for, so after
 * large moves a rebuild traverses faster (kitchen stand-in, one 1080p sub-frame's closest-hit trace: 2.2 ms as built, 2.9 ms after one instance moved by half
 * the room, 84 ms after every instance moved, 2.8 ms rebuilt).  Drops sub-frames traced ahead, as every scene setter does.  Cost: the shading tables, one
 * launch per tree level of every tree whose boxes changed, one host inversion per instance -- kitchen stand-in with every instance moved: 2.1 ms baked
 * (64-69 ms build), 0.6 ms with bake_world 0 (37 ms); 10^5 instances with bake_world 0: 1.3 ms (10.5 ms); docs/LOG.md. */
skh_status skh_update_accel(skh_context* ctx, const skh_instance* instances, uint32_t n_instances);

/* Which instances skh_build_accel baked to world space (option bake_world; `flags` receives one byte per instance, 1 = baked;
 * either pointer may be NULL).  A baked mesh instance has no IAS entry (OptixRender.cpp:412-441 creates one per instance): its
 * triangles are transformed once and intersected in world space.  Hit records name the same instance and primitive. */
skh_status skh_get_baked(skh_context* ctx, uint8_t* flags, uint32_t n_instances, uint32_t* out_baked_instances,
                         uint32_t* out_baked_triangles);

/* ---- updatePathtracerParams (OptixRender.cpp:827-872): (re)allocates accum/AOV buffers, resets history ---- */
skh_status skh_resize(skh_context* ctx, uint32_t width, uint32_t height);

/* Multi-GPU pixel-tile ownership (new; the reference is single-GPU).  tile_xy holds n_tiles (x0,y0)
 * pairs of tile_size x tile_size tiles this context renders; NULL / 0 = the whole image. */
skh_status skh_set_tiles(skh_context* ctx, uint32_t tile_size, const uint32_t* tile_xy, uint32_t n_tiles);

/* ---- OptiXRender::render's optixLaunch (OptixRender.cpp:1006-1021): one sub-frame batch.
 *      d_image may be NULL (only accum is updated).  Synchronous, like the reference: the image is complete when the call returns.
 *      Called once per sub-frame the library traces ahead (options speculate, speculate_async); the image is then written on a stream
 *      of the library's own that does NOT wait for the caller's null-stream work: d_image must have no writes of the caller's still
 *      pending when the call is made (the reference's callers only ever read it, RenderPass.cpp:441-447). ---- */
skh_status skh_render_subframe(skh_context* ctx, const skh_frame_params* params, void* d_image);
/* Called once per sub-frame, as HdStrelkaRenderPass::_Execute calls render() (RenderPass.cpp:441-447), the library traces ahead:
 * once two consecutive calls continue the same frame (identical parameters, subframe_index + 1) the next call traces 2, then 4,
 * ... up to option "speculate" (8) sub-frames in one wavefront pass, and the calls after it only apply their accumulation step.
 * The images are bit-identical to one-pass-per-call rendering (tests: test_speculative_subframes_are_exact); a call that does
 * not continue the frame -- camera motion restarts at sub-frame 0 -- simply discards what was traced ahead.  "speculate" 0 = off. */

/* Convenience for benchmarks: n consecutive sub-frames of params->samples_this_launch samples each,
 * starting at params->subframe_index, with a single device synchronisation at the end. */
skh_status skh_render_subframes(skh_context* ctx, const skh_frame_params* params, uint32_t n_subframes,
                                void* d_image);

/* ---- Adaptive sampling (new; the reference's only stopping rule is spp_total.  DESIGN.md section 2, "Adaptive sampling").
 *      Opt-in.  Every pixel keeps a Welford state {n, mean, M2} of the LDR luminance y = 0.2126 r + 0.7152 g + 0.0722 b of
 *      tonemap(observation, exposure), one observation per launch (the value the launch hands to the accumulator).  When the number of
 *      observations n since sub-frame 0 reaches min_samples, and every `interval` after that, each tile is checked:
 *      q = (M2 / n / n) / max(mean, dark_level)^2 per pixel, Q = the tile's largest q; the tile FREEZES iff Q <= threshold^2 (a NaN never
 *      freezes).  A frozen tile is not traced again in this frame and holds, bit for bit, the accumulator of the non-adaptive frame after as
 *      many launches.  The frame starts again -- all tiles active, statistics cleared -- at a call with subframe_index == 0 and after every
 *      scene setter, skh_resize and skh_set_tiles.  Acts only on calls with enable_accumulation != 0 and debug == 0.
 *      A context with adaptive sampling on renders one pass per skh_render_subframe call (nothing is traced ahead). ---- */
typedef struct skh_adaptive
{
    float threshold;      /* relative standard error at which a tile stops; finite, >= 0 */
    float dark_level;     /* LDR luminance below which the error is taken relative to this; finite, > 0 */
    uint32_t min_samples; /* >= 2 */
    uint32_t interval;    /* >= 1 */
    uint32_t reserved[4]; /* 0 */
} skh_adaptive;
/* SKH_OK when *a is a setting skh_set_adaptive accepts (needs no context and no GPU) */
skh_status skh_adaptive_check(const skh_adaptive* a);
/* NULL = off (the context then launches the kernels it launched before and frees the feature's buffers).  A setting that fails
 * skh_adaptive_check is refused with SKH_INVALID_ARGUMENT and the previous one stays. */
skh_status skh_set_adaptive(skh_context* ctx, const skh_adaptive* a);
typedef struct skh_adaptive_info
{
    uint32_t enabled;
    uint32_t tiles, active_tiles;
    uint32_t checks;                   /* done in this frame */
    uint32_t min_observations, max_observations; /* over the tiles: a frozen tile's count at its freeze, an active tile's count so far */
    uint64_t pixel_observations;       /* traced in this frame: valid pixels of active tiles, summed over the launches */
    uint64_t pixel_observations_saved; /* ... and those the frozen tiles did not trace, against the non-adaptive frame so far */
} skh_adaptive_info;
skh_status skh_get_adaptive_info(skh_context* ctx, skh_adaptive_info* out);
/* per pixel {n, mean, M2, q at the last check of its tile}; W*H float4, row-major; pixels of tiles this context does not own read as 0 */
skh_status skh_read_adaptive(skh_context* ctx, float* host_rgba);

/* ---- First-hit AOVs: what is under a pixel, and what the surface there looks like before lighting (new; DESIGN.md section 2, "First-hit AOVs").
 *      Hydra's primId / instanceId / elementId / depth AOVs, picking, and the normal / position / albedo buffers a denoiser or a sampling metric reads.
 *      A pass of its own, one ray per pixel of a region of the context's image, no accumulation, no anti-aliasing: a raw query, as skh_trace_device is.
 *   ray      pixel (px, py): generate_camera_ray(px, py, W, H, clip_to_view, view_to_world, jx, jy), W, H from skh_resize.  sample_index ==
 *            SKH_AOV_PIXEL_CENTRE: jx = jy = 0.5f.  Otherwise jx, jy = sampler_random(init_sampler(px, py, sample_index, spp_total, 52), DIM_PIXEL_X / DIM_PIXEL_Y):
 *            the camera ray skh_render_subframe traces for that sample, bit for bit -- the planes then describe the first hit of that sample's path.
 *            tmin from the parameters, tmax = 1e16f, closest hit.
 *   hit      what skh_trace_device(..., SKH_TRACE_CLOSEST) returns for that ray: cutouts honoured, blend hits under the raw-query rule (a > 0), cutout_rounds applies;
 *            independent of the builder and of every scheduling option; bake_world is part of its definition, as for every hit record.
 *   layout   plane k is a caller-owned device buffer of 16 * width * height bytes, pixel (x, y) at (y - y0) * width + (x - x0), row 0 = launch y 0 as for
 *            skh_read_accum.  A plane whose bit is clear is not touched and its pointer may be NULL.
 *   words    no fma: every product and sum is rounded, as everywhere in the library.
 *            kind         0 miss, 1 triangle of a mesh instance, 2 curve segment, 3 light proxy
 *            instance_id, prim_id   skh_hit's; 0xffffffff at a miss
 *            material     the index k_shade resolves (0xffffffff -> 0, beyond the list -> 0); 0xffffffff for kinds 0 and 3
 *            t, u, v      skh_hit's; at a miss t = -1, u = v = 0
 *            depth        clip = mul44(world_to_clip, (P, 1)) with P the POSITION plane's value, depth = clip.z / clip.w; 1 at a miss
 *            kind 1       P, N, Ng = fill_triangle(instance, w2o, record, u, v, inside = false): the reference's fillTriangleGeomData; N then replaced by the
 *                         normal-mapped normal exactly as k_shade does when the material's normal_texture is valid (the vector the debug = 1 view shows);
 *                         TEXCOORD = the interpolated text_coords[0]; ALBEDO = the material's base_color after resolve_material: what skh_material_probe answers
 *                         in out[0..2] for (material, u, v), for every material type
 *            kind 2       P, N = fill_curve(...): the reference's fillCurveGeomData, P being o + t * d moved into the curve's cross-section at the hit's u and onto the
 *                         radius there (what its normal function does to the point); Ng = N; TEXCOORD 0; ALBEDO = the material's base_color
 *            kinds 1, 2   facing = dot(Ng, -d) >= 0 ? 1 : -1, d the ray's direction
 *            kind 3       P = o + t * d (one product, one sum); N = Ng = 0, facing = 0; ALBEDO = (1, 1, 1, 1)
 *            kind 0       every float plane 0 (POSITION.w too), except the HIT plane's words above
 *   effects  none on the frame: the accumulator, the AOV accumulators and the adaptive statistics are not touched, tile ownership (skh_set_tiles) is ignored -- every
 *            context answers for the whole image --, rays_radiance / rays_shadow do not move (the rays are counted in skh_aov_info.rays).  Like skh_trace it waits for
 *            and drops sub-frames traced ahead: speculation is exact, so images do not change; the drop is counted in skh_stats.speculated_discarded.
 *   refused  with SKH_INVALID_ARGUMENT, nothing written, the previous state kept: a region that leaves the image or has exactly one zero side; planes == 0 or bits at
 *            or above SKH_AOV_COUNT; a set bit with a NULL pointer; a matrix entry that is not finite; tmin negative or not finite; with sample_index naming a
 *            sample, spp_total == 0 or sample_index >= spp_total (an index outside the sequence); a non-zero reserved word; no skh_resize yet.  Without an
 *            acceleration structure the call builds one, as skh_trace does.
 *   cost     the region is processed in bands of at most option aov_band rays (2^22; 64 ... 2^26): a 32-byte ray and a 20-byte hit record per ray of a band,
 *            freed before the call returns.  With option timing its spans are a class of their own: ms_trace_closest does not move.
 * Not part of it: accumulated or anti-aliased planes, authored face ids (prim_id is the triangle), the eye-space normal, multi-rank gathering.
 * Motion vectors come from skh_temporal (its d_motion plane), which reprojects these planes into the previous frame. */
#define SKH_AOV_IDS         0u /* uint32 x 4: instance_id, prim_id, material, kind */
#define SKH_AOV_HIT         1u /* float  x 4: t, u, v (skh_hit's), depth */
#define SKH_AOV_NORMAL      2u /* float  x 4: N.xyz, facing */
#define SKH_AOV_POSITION    3u /* float  x 4: P.xyz, 1 */
#define SKH_AOV_GEOM_NORMAL 4u /* float  x 4: Ng.xyz, 0 */
#define SKH_AOV_ALBEDO      5u /* float  x 4: rgb, 1 */
#define SKH_AOV_TEXCOORD    6u /* float  x 4: text_coords[0].u, .v, 0, 0 */
#define SKH_AOV_COUNT       7u
#define SKH_AOV_PIXEL_CENTRE 0xffffffffu

typedef struct skh_aov_params
{
    float view_to_world[16], clip_to_view[16]; /* as skh_frame_params: row-major */
    float world_to_clip[16];                   /* row-major; used by the depth word only */
    uint32_t x0, y0, width, height;            /* region of the context's image; width = height = 0: the whole image */
    uint32_t sample_index;                     /* SKH_AOV_PIXEL_CENTRE, or the sample whose camera ray is traced */
    uint32_t spp_total;                        /* the sampler's, when sample_index names a sample; else ignored */
    float tmin;                                /* finite, >= 0 */
    uint32_t reserved[5];                      /* 0 */
} skh_aov_params;

/* SKH_OK when *p is a setting skh_render_aovs accepts for an image of image_w x image_h pixels (needs no context and no GPU, as skh_adaptive_check) */
skh_status skh_aov_check(const skh_aov_params* p, uint32_t image_w, uint32_t image_h);
skh_status skh_render_aovs(skh_context* ctx, const skh_aov_params* p, uint32_t planes /* bit k = plane k */, void* const d_planes[SKH_AOV_COUNT]);
typedef struct skh_aov_info
{
    uint64_t calls, rays; /* since the last skh_reset_stats */
    double ms_last;       /* wall time of the last call, its synchronisation included */
    uint64_t bytes_last;  /* plane bytes the last call wrote */
} skh_aov_info;
skh_status skh_get_aov_info(skh_context* ctx, skh_aov_info* out);

/* ---- Denoiser: an edge-avoiding a-trous filter guided by the first-hit planes (new; DESIGN.md section 2, "Denoiser").  Dammertz et al., HPG 2010, with the
 *      position term taken as the tap's distance from the centre's tangent plane and the colour filtered after division by the first-hit albedo.
 *      The float32 planes below are the definition; what the kernels pack them into is a copy of their words.
 *   inputs   caller-owned device images of width x height records of 16 bytes, row-major, in the layout of skh_render_aovs: the colour C (float rgba), and the planes
 *            IDS (its `kind` word is used), NORMAL (xyz), POSITION (xyz), ALBEDO (rgb).
 *   surface  a SURFACE pixel has kind 1 or 2 and a colour whose r, g, b are finite.  Every other pixel (a miss, a light proxy, a non-finite colour) is copied to the
 *            output bit for bit and is never a tap of anybody else.  The alpha word of every pixel passes through bit for bit.
 *   level l  step s = 1 << l; for a surface pixel p, from the level's input c (the first level's: C, or C demodulated; then the previous level's output):
 *              taps   q = p + s (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner; a tap outside the image or on a pixel that is no surface pixel is skipped
 *              e = c(q) - c(p), n = N(q) - N(p), g = P(q) - P(p), each per component
 *              a = (((e.x e.x + e.y e.y) + e.z e.z) kc + ((n.x n.x + n.y n.y) + n.z n.z) kn) + (d d) kp,   d = (N(p).x g.x + N(p).y g.y) + N(p).z g.z
 *                  kc = 1 / (sc sc), sc = sigma_color 2^-l;  kn = 1 / (sigma_normal sigma_normal);  kp = 1 / (sigma_plane sigma_plane)   (float32; +inf gives 0)
 *              an a that is not <= 64 counts as 64 (a NaN too)
 *              w = (h[dx] h[dy]) exp(-a), h = {1/16, 1/4, 3/8, 1/4, 1/16}, exp = skh_libm.h's
 *              sw += w, sc += w c(q) per channel, in tap order;  out(p) = sc / sw per channel
 *            Every product, sum and quotient is a rounded float32 operation: no fma.  A skipped tap is selected out, never multiplied by zero (0 * NaN would
 *            poison the sum).  The order is fixed, so the bits are a function of the inputs alone.
 *   flags    SKH_DENOISE_DEMODULATE: the first level's input is C.rgb / m per channel on surface pixels, m = albedo > albedo_floor ? albedo : albedo_floor
 *            SKH_DENOISE_REMODULATE: the last level's output is multiplied by the same m.  Two flags, so that calls can be chained: levels first_level ..
 *            first_level + levels - 1 in one call give the bits of that many one-level calls, the first with DEMODULATE and the last with REMODULATE.
 *   call     synchronous, as skh_render_aovs.  d_out == d_color is allowed and gives the bits of the out-of-place call.  d_albedo may be NULL when neither flag
 *            is set.  params == NULL frees the scratch the context holds (the other arguments are ignored).
 *   effects  none on the frame: the accumulator, the AOV accumulators, the adaptive statistics and the ray counts are not read or written; tile ownership plays no
 *            part; sub-frames traced ahead are NOT dropped (the call reads nothing of the frame) -- it runs beside them, as skh_tonemap does.
 *   refused  with SKH_INVALID_ARGUMENT, nothing written, the previous state kept: what skh_denoise_check refuses -- width or height 0 or width * height > 2^26;
 *            levels 0 or first_level + levels > 8; a sigma that is <= 0 or NaN (+inf is legal and turns its term off); an albedo_floor that is <= 0 or not
 *            finite; a flag bit other than the two; a non-zero reserved word -- and a NULL image that the call needs.
 *   cost     scratch owned by the context, 56 bytes per pixel (two colour images, one guide record), grown when a larger image comes, freed by skh_destroy and
 *            by skh_denoise(ctx, NULL, ...).  A context that never calls it allocates and launches nothing for it.
 * Not part of it: separate diffuse / specular filtering, firefly clamping, a denoised accumulator.  Temporal accumulation and reprojection are a pass of their
 * own: skh_temporal, below; variance guidance (SVGF) is a call of its own: skh_denoise_variance, further below. */
#define SKH_DENOISE_DEMODULATE 1u
#define SKH_DENOISE_REMODULATE 2u
#define SKH_DENOISE_MAX_LEVEL  8u /* first_level + levels <= 8: steps up to 128 */

typedef struct skh_denoise_params
{
    uint32_t width, height;      /* >= 1, width * height <= 2^26 */
    uint32_t first_level, levels; /* levels >= 1, first_level + levels <= SKH_DENOISE_MAX_LEVEL */
    float sigma_color;           /* > 0 (+inf: off); of the first level's input, halved per level */
    float sigma_normal;          /* > 0 (+inf: off) */
    float sigma_plane;           /* > 0 (+inf: off); scene units */
    float albedo_floor;          /* finite, > 0 */
    uint32_t flags;              /* SKH_DENOISE_* */
    uint32_t reserved[7];        /* 0 */
} skh_denoise_params;

/* SKH_OK when *p is a setting skh_denoise accepts (needs no context and no GPU, as skh_aov_check) */
skh_status skh_denoise_check(const skh_denoise_params* p);
skh_status skh_denoise(skh_context* ctx, const skh_denoise_params* p, const void* d_color, const void* d_ids, const void* d_normal, const void* d_position,
                       const void* d_albedo, void* d_out);
typedef struct skh_denoise_info
{
    uint64_t calls, pixels;  /* since the last skh_reset_stats */
    double ms_last;          /* wall time of the last call, its synchronisation included */
    uint64_t scratch_bytes;  /* device bytes the context holds for the filter now */
} skh_denoise_info;
skh_status skh_get_denoise_info(skh_context* ctx, skh_denoise_info* out);

/* ---- Temporal accumulation: the previous frame's history, reprojected through the first-hit planes and blended with the new frame (new; DESIGN.md
 *      section 2, "Temporal accumulation").  A pure function of caller-owned device planes, one pass, one kernel (skh_temporal.h).
 *   inputs   caller-owned device images of width x height records of 16 bytes, row-major, in the layout of skh_render_aovs.  Of the current frame: the colour C
 *            (float rgba) and the planes IDS (instance_id and kind are used), NORMAL (xyz), POSITION (xyz), ALBEDO (rgb).  Of the previous frame: IDS, NORMAL,
 *            POSITION and a HISTORY record {illumination.rgb, n} per pixel, n the history length as a float.
 *   surface  skh_denoise's rule: kind 1 or 2 and finite r, g, b in C.  For every other pixel d_out is C bit for bit, d_history_out is {0, 0, 0, 0} and d_motion
 *            is {0, 0, 0, 0}.  The alpha word of d_out is C's, bit for bit, for every pixel.
 *   input    c = C.rgb; with SKH_TEMPORAL_DEMODULATE c = C.rgb / m per channel, m = albedo > albedo_floor ? albedo : albedo_floor (skh_denoise's rule: a NaN
 *            albedo gives the floor).  The history is kept in these units.
 *   project  clip = mul44(prev_world_to_clip, (P, 1)), P = POSITION(p).xyz, each row ((m0 P.x + m1 P.y) + m2 P.z) + m3 1;
 *            fx = ((clip.x / clip.w) 0.5 + 0.5) W - 0.5, fy = ((clip.y / clip.w) 0.5 + 0.5) H - 0.5: the inverse of generate_camera_ray's
 *            ndc = (px + 0.5) / W 2 - 1, no y flip.  The pixel PROJECTS iff clip.w > 0 and fx, fy are finite with -1 <= fx <= W and -1 <= fy <= H; the range
 *            test comes before any conversion to an integer.
 *   taps     ix = floor(fx), tx = fx - ix, likewise in y; q_k = (ix + dx, iy + dy) for (dx, dy) = (0,0), (1,0), (0,1), (1,1), with the weights
 *            (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty.  Tap k is ACCEPTED iff it lies in the image, its weight is > 0, the previous IDS there has the
 *            kind and the instance_id of the current pixel, the previous history there has finite rgb and a finite n >= 1,
 *            (N'(q).x N(p).x + N'(q).y N(p).y) + N'(q).z N(p).z >= normal_min, and |d| <= plane_tolerance with g = P'(q) - P(p) per component and
 *            d = (N(p).x g.x + N(p).y g.y) + N(p).z g.z (skh_denoise's d).  Every comparison is written so that a NaN rejects.  A rejected tap is selected
 *            out, never multiplied by zero; an address outside the image is clamped to a legal one before the load.
 *   blend    with an accepted tap, in tap order: sw = sum w, h = sum (w hist.rgb) / sw, nh = sum (w hist.n) / sw, n' = min(nh + 1, max_history),
 *            alpha = 1 / n', ill = h + (c - h) alpha per channel.  Otherwise (the pixel does not project, or no tap is accepted) ill = c, n' = initial_length.
 *            d_history_out = {ill, n'};  d_out.rgb = ill m with DEMODULATE, else ill.
 *            Every product, sum and quotient is a rounded float32 operation: no fma.  The order is fixed, so the bits are a function of the inputs alone.
 *   motion   d_motion, when not NULL: {fx - px, fy - py, sw, mask}, mask a float holding bit k for an accepted tap k (0 ... 15).  A surface pixel that does not
 *            project writes {0, 0, 0, 0}; one that projects without an accepted tap writes its motion with sw = 0, mask = 0.
 *   no prev  d_prev_history == NULL: there is no previous frame.  The other three previous-frame pointers and the matrix's use are dropped, and every surface
 *            pixel takes the branch without history: how a host seeds a history of a known length (initial_length).
 *   call     synchronous, on the stream skh_denoise uses.  d_out == d_color is allowed (a pixel reads only its own C) and gives the bits of the out-of-place
 *            call; d_history_out == d_prev_history is refused (taps read neighbours).  d_albedo may be NULL without DEMODULATE.
 *   effects  none on the frame: the accumulator, the AOV accumulators, the adaptive statistics and the ray counts are not read or written; tile ownership plays
 *            no part; sub-frames traced ahead are not dropped.  No scratch memory: a context that never calls it allocates and launches nothing for it.
 *   refused  with SKH_INVALID_ARGUMENT, nothing written, the previous state kept: what skh_temporal_check refuses -- width or height 0 or width * height >
 *            2^26; a matrix entry that is not finite; normal_min outside [-1, 1] or NaN; plane_tolerance <= 0 or NaN (+inf is legal and turns the test off);
 *            max_history not finite or < 1; initial_length not finite, < 1 or > max_history; an albedo_floor that is <= 0 or not finite; a flag bit other than
 *            DEMODULATE; a non-zero reserved word -- and a NULL image that the call needs, and the alias above.
 * Object motion: the call projects P as if nothing in the world had moved.  For moved instances hand it, as d_normal and d_position, the planes that
 * skh_rewind_guides (further below) writes.
 * Lighting changes: a tap is accepted on geometry alone; skh_rectify (further below) clamps the history this call wrote to a fast history's window.
 * Not part of it: separate diffuse / specular histories (luminance moments and variance guidance: skh_moments, below), what is seen in mirrors
 * and through glass (the guides describe the first surface). */
#define SKH_TEMPORAL_DEMODULATE 1u

typedef struct skh_temporal_params
{
    uint32_t width, height;       /* >= 1, width * height <= 2^26 */
    float prev_world_to_clip[16]; /* row-major: the world_to_clip of the skh_aov_params the previous guide planes were rendered with */
    float normal_min;             /* in [-1, 1]: the least dot of the two normals */
    float plane_tolerance;        /* > 0 (+inf: off); scene units */
    float max_history;            /* finite, >= 1: alpha never falls below 1 / max_history */
    float initial_length;         /* finite, in [1, max_history]: the n' of a pixel without history */
    float albedo_floor;           /* finite, > 0 */
    uint32_t flags;               /* SKH_TEMPORAL_* */
    uint32_t reserved[8];         /* 0 */
} skh_temporal_params;

/* SKH_OK when *p is a setting skh_temporal accepts (needs no context and no GPU, as skh_denoise_check) */
skh_status skh_temporal_check(const skh_temporal_params* p);
skh_status skh_temporal(skh_context* ctx, const skh_temporal_params* p, const void* d_color, const void* d_ids, const void* d_normal, const void* d_position,
                        const void* d_albedo, const void* d_prev_history, const void* d_prev_ids, const void* d_prev_normal, const void* d_prev_position,
                        void* d_out, void* d_history_out, void* d_motion /* may be NULL */);
typedef struct skh_temporal_info
{
    uint64_t calls, pixels; /* since the last skh_reset_stats */
    double ms_last;         /* wall time of the last call, its synchronisation included */
} skh_temporal_info;
skh_status skh_get_temporal_info(skh_context* ctx, skh_temporal_info* out);

/* ---- Variance guidance: luminance moments carried through skh_temporal's reprojection, and an a-trous filter whose luminance edge-stop is scaled by the
 *      local standard deviation (new; DESIGN.md section 2, "Variance guidance").  Schied et al., HPG 2017 (SVGF).  Two pure functions of caller-owned device
 *      planes (skh_variance.h); records, row order, rounding (every product, sum, quotient and square root one rounded float32 operation, no fma; sqrtf is
 *      correctly rounded), the fixed summation order, selection of skipped taps, clamped addresses and NaN-failing comparisons are skh_denoise's and
 *      skh_temporal's.  lum(c) = (0.2126f c.x + 0.7152f c.y) + 0.0722f c.z.  SURFACE is skh_denoise's rule, m its albedo floor rule.
 *
 *   skh_moments   MOMENTS record {mu1, mu2, variance, nm}, nm the moments' own history length as a float.  p is the struct given to skh_temporal for this
 *            frame (checked by skh_temporal_check; normal_min and plane_tolerance are not used); d_color .. d_albedo are the current frame's as handed to
 *            skh_temporal (the RAW colour, not its output); d_motion is the motion plane that call wrote.
 *              a pixel that is no surface pixel writes {0, 0, 0, 0}
 *              l = lum(c), c = C.rgb, or C.rgb / m with SKH_TEMPORAL_DEMODULATE
 *              with a previous frame (d_motion and d_prev_moments given): fx, fy, PROJECTS, the four taps and their weights are skh_temporal's, recomputed from
 *              POSITION(p) and p->prev_world_to_clip; mask = (motion.w >= 0 && motion.w <= 15) ? (uint)motion.w : 0.  Tap k is USED iff the pixel projects, bit k
 *              of mask is set, the tap lies in the image, its weight is > 0, and the previous MOMENTS there has finite mu1, mu2 and a finite nm >= 1.
 *              with a used tap, in tap order: sw = sum w, m1 = sum (w mu1) / sw, m2 = sum (w mu2) / sw, nh = sum (w nm) / sw, nm' = min(nh + 1, max_history),
 *              alpha = 1 / nm', mu1' = m1 + (l - m1) alpha, mu2' = m2 + (l l - m2) alpha.  Otherwise mu1' = l, mu2' = l l, nm' = initial_length.
 *              v = mu2' - mu1' mu1'; variance = v > 0 ? v : 0.
 *            Refused as skh_temporal refuses, and: d_moments_out == d_prev_moments, or exactly one of d_motion / d_prev_moments NULL.  No scratch, no effect
 *            on the frame, synchronous on skh_denoise's stream.
 *
 *   skh_denoise_variance   skh_denoise with the colour term replaced by a luminance term and the variance filtered along.  d_moments is a MOMENTS plane.
 *     input variance  v0(p) = z when z = MOMENTS(p).variance is finite and > 0, else 0.  With SKH_VDENOISE_ESTIMATE a surface pixel whose nm is not >= min_history
 *            takes the spatial estimate instead: over dy = -3 .. 3 outer, dx = -3 .. 3 inner, step 1, the taps that lie in the image, are surface pixels and have
 *            finite mu1, mu2: w = exp(-(a <= 64 ? a : 64)), a = tn + tp (skh_denoise's normal and plane terms), s0 += w, s1 += w mu1(q), s2 += w mu2(q);
 *            e1 = s1 / s0, e2 = s2 / s0, v = e2 - e1 e1, v = v > 0 ? v : 0, k = min_history / (nm >= 1 ? nm : 1), v0 = v k.  No used tap gives 0.
 *     level l  step 1 << l.  For a surface pixel p, from the level's input colour c and variance v:
 *              vbar(p) = the 3 x 3 Gaussian {1/16, 1/8, 1/16; 1/8, 1/4, 1/8; 1/16, 1/8, 1/16} of v over the surface taps in the image at offsets -1 .. 1 (not
 *              dilated), dy outer, dx inner: sum (k v(q)) / sum k over the taps taken
 *              kl = 1 / (sigma_luminance sqrtf(vbar) + epsilon)
 *              per tap of skh_denoise's 5 x 5: tl = fabsf(lum(c(q)) - lum(c(p))) kl (with sigma_luminance == +inf tl is 0: selected, not computed as inf 0);
 *              a = (tl + tn) + tp; an a that is not <= 64 counts as 64; w = (h[dx] h[dy]) exp(-a)
 *              sw += w, sc += w c(q) per channel, sv += (w w) v(q);  out = sc / sw, v_out = sv / (sw sw): the next level's c and v
 *     flags    DEMODULATE / REMODULATE as in skh_denoise; the variance is in the first level's (demodulated) units throughout and is never remodulated.
 *            Pixels that are no surface pixels and every alpha word are copied bit for bit.
 *     d_moments_out  when not NULL: {mu1, mu2, v_out of the last level, nm} on surface pixels, mu1, mu2, nm copied from d_moments; {0, 0, 0, 0} elsewhere.
 *            Feeding it to the next call without ESTIMATE makes the levels of one call equal chained one-level calls, bit for bit, on both outputs.
 *            d_out == d_color and d_moments_out == d_moments are allowed.
 *     refused  what skh_vdenoise_check refuses -- skh_denoise's clauses for the shared fields, an epsilon that is <= 0 or not finite, a min_history that is < 1
 *            or not finite, an unknown flag bit, a non-zero reserved word -- and a NULL image that the call needs, d_moments among them.
 *     cost     the scratch is skh_denoise's allocation (56 bytes per pixel, the variance rides in the colour record's fourth word): both calls grow it, both free
 *            it with params == NULL, skh_get_denoise_info and skh_get_vdenoise_info report the same bytes.
 * Not part of it: separate diffuse / specular histories, neighbourhood colour clamping, feeding the first level's output back into the history, variance for a
 * still camera's accumulator, multi-rank handling beyond "rank 0 on the gathered image". */
#define SKH_VDENOISE_ESTIMATE 4u

skh_status skh_moments(skh_context* ctx, const skh_temporal_params* p, const void* d_color, const void* d_ids, const void* d_position, const void* d_albedo,
                       const void* d_motion /* NULL = no previous frame */, const void* d_prev_moments /* NULL = no previous frame */, void* d_moments_out);
typedef struct skh_moments_info
{
    uint64_t calls, pixels; /* since the last skh_reset_stats */
    double ms_last;         /* wall time of the last call, its synchronisation included */
} skh_moments_info;
skh_status skh_get_moments_info(skh_context* ctx, skh_moments_info* out);

typedef struct skh_vdenoise_params
{
    uint32_t width, height;       /* as skh_denoise_params */
    uint32_t first_level, levels; /* as skh_denoise_params */
    float sigma_luminance;        /* > 0 (+inf: the term is off); in standard deviations of the luminance */
    float sigma_normal;           /* > 0 (+inf: off) */
    float sigma_plane;            /* > 0 (+inf: off); scene units */
    float albedo_floor;           /* finite, > 0 */
    float epsilon;                /* finite, > 0; luminance units */
    float min_history;            /* finite, >= 1 */
    uint32_t flags;               /* SKH_DENOISE_DEMODULATE | SKH_DENOISE_REMODULATE | SKH_VDENOISE_ESTIMATE */
    uint32_t reserved[5];         /* 0 */
} skh_vdenoise_params;

/* SKH_OK when *p is a setting skh_denoise_variance accepts (needs no context and no GPU, as skh_denoise_check) */
skh_status skh_vdenoise_check(const skh_vdenoise_params* p);
skh_status skh_denoise_variance(skh_context* ctx, const skh_vdenoise_params* p, const void* d_color, const void* d_ids, const void* d_normal,
                                const void* d_position, const void* d_albedo, const void* d_moments, void* d_out, void* d_moments_out /* may be NULL */);
typedef struct skh_vdenoise_info
{
    uint64_t calls, pixels;  /* since the last skh_reset_stats */
    double ms_last;          /* wall time of the last call, its synchronisation included */
    uint64_t scratch_bytes;  /* device bytes the context holds for the filter now (skh_denoise_info's) */
} skh_vdenoise_info;
skh_status skh_get_vdenoise_info(skh_context* ctx, skh_vdenoise_info* out);

/* ---- Object motion: the current frame's POSITION and NORMAL planes rewound into the previous frame's world, so that skh_temporal and skh_moments follow
 *      instances whose transforms changed between the two frames (new; DESIGN.md section 2, "Object motion").  skh_temporal uses the current POSITION and NORMAL
 *      for the projection, the normal test against N'(q) and the plane test against P'(q); skh_moments uses POSITION for the projection.  Handed where the
 *      surface point WAS and how it FACED, each of those uses is right as it stands.  One pass, one kernel (skh_motion.h), and the table that drives it.
 *
 *   table    skh_instance_motion per instance, indexed by IDS.instance_id.  to_prev maps a current world position of the instance to its previous one,
 *            normal_to_prev a current world normal to a positive multiple of its previous one.  SKH_MOTION_MOVED: the matrices apply; without it the entry
 *            is skipped and its matrix words are not looked at.  SKH_MOTION_DROP (with MOVED): the instance's pixels get no history.
 *   skh_instance_motion_from_transforms   the single place an entry is derived: from the instance's 3 x 4 row-major transforms (object to world, as
 *            skh_set_instances takes them) of the previous frame, A = [A_lin | a], and of the current one, B = [B_lin | b].  Host only; needs no context and
 *            no GPU.  When the twelve words of A and B are equal bit for bit: flags = 0, identity matrices.  Otherwise, in double, each operation rounded once,
 *            in this order:
 *              inv(M), M 3 x 3:  c00 = m11 m22 - m12 m21, c01 = m12 m20 - m10 m22, c02 = m10 m21 - m11 m20, det = (m00 c00 + m01 c01) + m02 c02;
 *                       the adjugate's entry (i, j) = m[j+1][i+1] m[j+2][i+2] - m[j+1][i+2] m[j+2][i+1] with the indices taken modulo 3 (c00, c01, c02 are its
 *                       first column); inv(M)(i, j) = adjugate(i, j) / det
 *              Bi = inv(B_lin), Ai = inv(A_lin)
 *              L(i, j) = (A_lin(i, 0) Bi(0, j) + A_lin(i, 1) Bi(1, j)) + A_lin(i, 2) Bi(2, j)
 *              t(i) = a(i) - ((L(i, 0) b(0) + L(i, 1) b(1)) + L(i, 2) b(2))
 *              K(i, j) = (Ai(0, i) B_lin(j, 0) + Ai(1, i) B_lin(j, 1)) + Ai(2, i) B_lin(j, 2): transpose(inv(A_lin)) transpose(B_lin), the inverse transpose of
 *                       L itself and not its cofactor matrix, so that a mirror keeps its sign
 *            to_prev = [L | t] and normal_to_prev = K, each entry rounded once to float32; flags = MOVED.  When either determinant is 0, or an input word or a
 *            rounded word is not finite: flags = MOVED | DROP and identity matrices.  SKH_INVALID_ARGUMENT for a NULL pointer, nothing else fails.
 *   skh_instance_motion_check   refuses a flag bit other than the two, DROP without MOVED, a non-zero reserved word, a matrix word that is not finite in an
 *            entry that is MOVED and not DROP, and table == NULL with n > 0.  Needs no context and no GPU.
 *   skh_set_instance_motion   checks the table and uploads it into a device table the context owns; the table grows when a larger one comes and is freed by
 *            n == 0 and by skh_destroy.  It is an input of its own: no scene setter touches it and it touches no derived state (it is no entry of the
 *            staleness table).  A refused table leaves the previous one in force.
 *   skh_rewind_guides   a pure function of caller-owned planes in the layout of skh_render_aovs; records, row order and rounding are skh_temporal's: every
 *            product, sum, quotient and square root is one rounded float32 operation, no fma.  Per pixel, id = IDS, P = POSITION, N = NORMAL; the entry
 *            e = table[id.instance_id] APPLIES iff id.kind is 1 or 2, id.instance_id < n and e.flags & MOVED.  With m = e.to_prev, k = e.normal_to_prev:
 *              applies, no DROP   P*.x = ((m0 P.x + m1 P.y) + m2 P.z) + m3, rows y (m4 ..) and z (m8 ..) likewise
 *                                 v.x = (k0 N.x + k1 N.y) + k2 N.z, rows y (k3 ..) and z (k6 ..) likewise; s = (v.x v.x + v.y v.y) + v.z v.z; N* = v / sqrtf(s)
 *                                 per component.  No special case: a zero or NaN normal gives a NaN N*, which skh_temporal's NaN-failing comparisons reject
 *                                 (a NaN that an operation produces has no defined payload; a copied word keeps its bits).
 *              applies, DROP      P*.xyz = the quiet NaN 0x7fc00000 (skh_temporal and skh_moments find that the pixel does not project); N* = N
 *              the .w words of both planes pass through
 *              every other pixel  both records copied bit for bit
 *            d_position_out == d_position and d_normal_out == d_normal are allowed (a pixel reads only its own records) and give the bits of the out-of-place
 *            call.  Synchronous, on the stream skh_denoise uses.  No effect on the frame, sub-frames traced ahead are not dropped, no scratch beyond the table.
 *            Refused with SKH_INVALID_ARGUMENT, nothing written: width or height 0 or width * height > 2^26, a NULL plane, no table set.
 *   use      rewind the current frame's planes, hand the rewound pair to skh_temporal (d_normal, d_position) and to skh_moments (d_position); its motion plane
 *            then follows the instance too.  skh_denoise, skh_denoise_variance and the NEXT frame's previous guides keep the true planes.
 * Not part of it: the shadow (or reflection, or bounce light) a moved object casts on OTHER surfaces lags as any lighting change does; deforming meshes (vertex
 * edits followed by skh_refit_accel have no per-instance motion); what is seen in mirrors and through glass (the guides describe the first surface). */
#define SKH_MOTION_MOVED 1u /* the entry's matrices apply */
#define SKH_MOTION_DROP 2u  /* with MOVED: the instance's pixels get no history (replaced, teleported, singular transform) */
typedef struct skh_instance_motion /* 96 bytes, six float4 */
{
    float to_prev[12];       /* row-major 3x4: P_prev = to_prev (P, 1) */
    float normal_to_prev[9]; /* row-major 3x3: N_prev ~ normal_to_prev N (any positive scale) */
    uint32_t flags;          /* SKH_MOTION_* */
    uint32_t reserved[2];    /* 0 */
} skh_instance_motion;

skh_status skh_instance_motion_from_transforms(const float prev[12], const float cur[12], skh_instance_motion* out);
skh_status skh_instance_motion_check(const skh_instance_motion* table, uint32_t n);
skh_status skh_set_instance_motion(skh_context* ctx, const skh_instance_motion* table, uint32_t n);
skh_status skh_rewind_guides(skh_context* ctx, uint32_t width, uint32_t height, const void* d_ids, const void* d_position, const void* d_normal,
                             void* d_position_out, void* d_normal_out);
typedef struct skh_rewind_info
{
    uint64_t calls, pixels; /* since the last skh_reset_stats */
    double ms_last;         /* wall time of the last call, its synchronisation included */
    uint64_t entries;       /* entries of the table in force (0: none) */
} skh_rewind_info;
skh_status skh_get_rewind_info(skh_context* ctx, skh_rewind_info* out);

/* ---- History rectification: the long history skh_temporal wrote, clamped per pixel and channel to the mean +- k standard deviations of a second, short
 *      ("fast") history over a small window on the same surface (new; DESIGN.md section 2, "History rectification").  skh_temporal accepts a tap on geometry
 *      alone, so a surface whose LIGHTING changed (the shadow of an instance that moved) keeps the old light for max_history frames.  The fast history is what
 *      the same skh_temporal writes with a small max_history from a previous fast history; it follows such a change within a few frames, and the long one keeps
 *      its low noise wherever the two agree.  A pure function of caller-owned device planes, one pass, one kernel (skh_rectify.h).  Records, row order and
 *      rounding are skh_temporal's: every product, sum, difference, quotient and square root is one rounded float32 operation, no fma; sqrtf is correctly
 *      rounded; every comparison is written so that a NaN fails it; a skipped tap is selected out, never multiplied by zero; an address outside the image is
 *      clamped to a legal one before the load.
 *   inputs   d_image the image skh_temporal wrote (float rgba), IDS (instance_id and kind are used), ALBEDO (rgb; REMODULATE only), HISTORY the long history
 *            skh_temporal wrote, {ill.rgb, n}, and FAST the fast history, the same record {f.rgb, nf}.
 *   rectified   pixel p is RECTIFIED iff IDS(p).kind is 1 or 2, HISTORY(p) has finite rgb and a finite n >= 1, and FAST(p) has finite rgb and a finite nf >= 1.
 *            Every other pixel copies d_image to d_out and d_history to d_history_out bit for bit and writes d_info as {0, 0, 0, 0}.  The alpha word of d_out is
 *            d_image's, bit for bit, for every pixel.
 *   window   dy = -radius ... radius outer, dx = -radius ... radius inner, step 1.  Tap q = p + (dx, dy) is TAKEN iff it lies in the image, IDS(q) has the kind and
 *            the instance_id of IDS(p), and FAST(q) has finite rgb and a finite nf >= 1.  The centre of a rectified pixel is always taken, so s0 >= 1.
 *   statistics   per channel, f = FAST(q)'s channel, two sweeps over the taken taps in that order:
 *              first   s0 = s0 + 1, s1 = s1 + f;  mean = s1 / s0
 *              second  d = f - mean, s2 = s2 + d d;  sd = sqrtf(s2 / s0)
 *            (two sweeps and not sum f f - mean mean, whose cancellation has no honest error bar; how the second sweep gets at f is the kernel's business)
 *   clamp    h = HISTORY(p)'s channel.  e = k sd, lo = mean - e, hi = mean + e;  r = h;  r = h < lo ? lo : r;  r = h > hi ? hi : r.  Bit c of mask (c = 0, 1, 2
 *            for r, g, b) is set where h < lo or h > hi.  With k == +inf neither comparison is made: r = h, mask = 0 (selected, not computed as inf 0).
 *   length   n' = n;  with SKH_RECTIFY_SHORTEN, mask != 0 and nf(p) < n:  n' = nf(p)
 *   outputs  d_history_out = {r, n'};  d_out.rgb = r m with SKH_RECTIFY_REMODULATE, else r, m = albedo > albedo_floor ? albedo : albedo_floor (skh_denoise's
 *            rule).  skh_temporal computes ill m in the same way, so an unclamped pixel's d_out has d_image's bits.
 *            d_info, when not NULL: {(float)mask, s0, dmax, n'}, dmax = |r - h| of r, then g and b each replacing it where larger (a > comparison).
 *   call     synchronous, on the stream skh_denoise uses.  d_out == d_image and d_history_out == d_history are allowed (a pixel reads only its own records of
 *            those planes) and give the bits of the out-of-place call; d_history_out == d_fast and d_out == d_fast are refused (the window reads neighbours).
 *            d_albedo may be NULL without REMODULATE.
 *   effects  none on the frame: the accumulator, the AOV accumulators, the adaptive statistics and the ray counts are not read or written; sub-frames traced
 *            ahead are not dropped.  No scratch memory: a context that never calls it allocates and launches nothing for it.
 *   refused  with SKH_INVALID_ARGUMENT, nothing written, the previous state kept: what skh_rectify_check refuses -- width or height 0 or width * height >
 *            2^26; a radius outside 1 ... 3; k <= 0 or NaN; an albedo_floor that is <= 0 or not finite; a flag bit other than the two; a non-zero reserved
 *            word -- and a NULL image that the call needs, and the two aliases above.
 * Not part of it: the moments of skh_moments stay unrectified (their variance lags a lighting change as the history did); what is seen in mirrors and through
 * glass (the guides describe the first surface); deforming meshes. */
#define SKH_RECTIFY_REMODULATE 1u /* d_out.rgb = r m */
#define SKH_RECTIFY_SHORTEN 2u    /* a clamped pixel's history is no longer than its fast history */

typedef struct skh_rectify_params
{
    uint32_t width, height; /* >= 1, width * height <= 2^26 */
    uint32_t radius;        /* 1, 2 or 3: a 3 x 3, 5 x 5 or 7 x 7 window */
    float k;                /* > 0; +inf is legal and clamps nothing */
    float albedo_floor;     /* finite, > 0 */
    uint32_t flags;         /* SKH_RECTIFY_* */
    uint32_t reserved[8];   /* 0 */
} skh_rectify_params;

/* SKH_OK when *p is a setting skh_rectify accepts (needs no context and no GPU, as skh_temporal_check) */
skh_status skh_rectify_check(const skh_rectify_params* p);
skh_status skh_rectify(skh_context* ctx, const skh_rectify_params* p, const void* d_image, const void* d_ids, const void* d_albedo /* may be NULL */,
                       const void* d_history, const void* d_fast, void* d_out, void* d_history_out, void* d_info /* may be NULL */);
typedef struct skh_rectify_info
{
    uint64_t calls, pixels; /* since the last skh_reset_stats */
    double ms_last;         /* wall time of the last call, its synchronisation included */
} skh_rectify_info;
skh_status skh_get_rectify_info(skh_context* ctx, skh_rectify_info* out);

/* ---- the tonemap() + gammaCorrection post pass (postprocessing/Tonemappers.cu:111-135), in place on a
 *      device float4 image.  type: 0 none, 1 Reinhard, 2 ACES fitted, 3 ACES film; gamma <= 0 = off ---- */
skh_status skh_tonemap(skh_context* ctx, void* d_image, uint32_t width, uint32_t height, uint32_t type,
                       const float exposure[3], float gamma);

/* ---- device image buffers: OptixBuffer's cudaMalloc / cudaFree / cudaMemcpy (OptixBuffer.cpp:16-43, 45-63) ---- */
skh_status skh_buffer_alloc(skh_context* ctx, size_t bytes, void** out_device_ptr);
skh_status skh_buffer_free(skh_context* ctx, void* device_ptr);
skh_status skh_buffer_download(skh_context* ctx, const void* device_ptr, void* host, size_t bytes);
/* host -> device, the mirror of skh_buffer_download: how a caller hands planes of its own (skh_denoise's inputs, say) to the device.  Synchronous. */
skh_status skh_buffer_upload(skh_context* ctx, void* device_ptr, const void* host, size_t bytes);
/* Page-locks / releases a caller-owned host range so that skh_buffer_download into it runs at PCIe rate (the host mirror of
 * Buffer::map, OptixBuffer.cpp:37-43, is a pageable std::vector in the reference; the caller maps after EVERY sub-frame). */
skh_status skh_host_register(skh_context* ctx, void* host, size_t bytes);
skh_status skh_host_unregister(skh_context* ctx, void* host);

/* ---- read-back: Buffer::map (OptixBuffer.cpp:37-43) ---- */
skh_status skh_read_accum(skh_context* ctx, float* host_rgba); /* W*H float4, row-major, row 0 = launch y 0 */
skh_status skh_read_aov(skh_context* ctx, uint32_t which /*0 diffuse, 1 specular*/, float* host_rgba);
skh_status skh_copy_accum(skh_context* ctx, void* d_dst_rgba); /* device-to-device, W*H float4 */
/* the diffuse (0) / specular (1) AOV accumulator, device-to-device: what render() copies to the image when all samples are done and
 * the debug view is 2 / 3 (OptixRender.cpp:1029-1042) */
skh_status skh_copy_aov(skh_context* ctx, uint32_t which, void* d_dst_rgba);
/* compact tile accumulators of this context: n_tiles * tile_size^2 float4, tile-major (for the RCCL gather) */
skh_status skh_copy_accum_tiles(skh_context* ctx, void* d_dst);
/* scatter gathered compact tiles into a W*H float4 image (root side of the gather) */
skh_status skh_scatter_tiles(skh_context* ctx, const void* d_src_tiles, const uint32_t* tile_xy, uint32_t n_tiles,
                             uint32_t tile_size, void* d_dst_rgba, uint32_t width, uint32_t height);

/* ---- multi-GPU: the one collective of a tile-sharded frame, below the C ABI (RCCL over xGMI; the reference is single-GPU,
 *      include/render/render.h:19-56 has no counterpart).  One communicator per context, bootstrapped the NCCL way: rank 0
 *      calls skh_comm_unique_id, the host distributes the 128 bytes (pipe, file, MPI, torch.distributed ...), every rank
 *      calls skh_comm_init (collective).  skh_gather_tiles: every rank's compact tile accumulators (the layout of
 *      skh_copy_accum_tiles, zero-padded to max_tiles tiles) -> the root's d_recv = [world][max_tiles][tile_size^2] float4, as
 *      ONE group of point-to-point sends into the root on the context's stream -- each sender uses its own xGMI link, no ring.
 *      Synchronous like render().  world_size 1 needs no communicator (a device-to-device copy).  librccl is loaded on first
 *      use; a box without it gets SKH_FAIL from skh_comm_*, nothing else depends on it. ---- */
#define SKH_COMM_ID_BYTES 128
skh_status skh_comm_unique_id(void* out_id /* SKH_COMM_ID_BYTES */);
skh_status skh_comm_init(skh_context* ctx, const void* id, int world_size, int rank);
skh_status skh_comm_destroy(skh_context* ctx);
/* world size / rank of the context's communicator and the rank count RCCL itself reports for it (ncclCommCount; 0 = none) */
skh_status skh_comm_info(skh_context* ctx, int* out_world_size, int* out_rank, int* out_rccl_ranks);
skh_status skh_gather_tiles(skh_context* ctx, uint32_t max_tiles, void* d_recv /* root only, else NULL */, int root);

/* ---- ray queries against the built accel (the optixTrace call sites), for tests and micro-benchmarks.
 *      rays/hits are HOST arrays. ---- */
skh_status skh_trace(skh_context* ctx, const skh_ray* rays, uint32_t n_rays, uint32_t mode, skh_hit* hits);
/* same on caller-owned DEVICE arrays (skh_ray / skh_hit records), the traversal repeated `repeat` times (micro-benchmarks);
 * returns once the hits are in d_hits */
skh_status skh_trace_device(skh_context* ctx, const void* d_rays, uint32_t n_rays, uint32_t mode, void* d_hits,
                            uint32_t repeat);

/* ---- memory ceilings of this GPU, measured with the access shapes of the hot path ("report a measured STREAM-copy
 *      ceiling"; the reference has no counterpart).  bench.py puts them beside the roofline fractions.  `bytes` = size of the
 *      probed buffer (allocated and freed inside; COPY takes two).  COPY: uint4 grid-stride copy, rate counts read + write.
 *      GATHER / CHASE: one-wave workgroups on the trace kernels' grid, every lane fetches 256 pseudo-random aligned records of
 *      record_bytes (32, 64 = one BVH node, or 128 = one cache line) -- four independent fetches in flight, or each address taken
 *      from the record before it (a traversal step); rate = record_bytes x fetches / time, whatever cache level served them. ---- */
#define SKH_PROBE_COPY 0u
#define SKH_PROBE_GATHER 1u
#define SKH_PROBE_CHASE 2u
skh_status skh_probe_memory(skh_context* ctx, uint32_t kind, uint64_t bytes, uint32_t record_bytes, uint32_t repeat, double* out_gbps,
                            double* out_ms);

/* ---- BSDF probes for tests: mdlcode_sample and mdlcode_evaluate (the call protocol of closest_hit.cu:563-605) run on the
 *      device for n independent inputs against the context's material list; host arrays.  One query = one MDL state
 *      (normal, geom_normal, tangent_u[0]) + k1 + the four xi of sample() + the k2 handed to evaluate(). ---- */
typedef struct skh_bsdf_query
{
    float normal[3], geom_normal[3], tangent_u[3];
    float k1[3]; /* outgoing direction (= -ray direction) */
    float k2[3]; /* incoming direction for evaluate() */
    float xi[4];
    uint32_t material; /* index into the list set by skh_set_materials */
    uint32_t inside; /* selects ior1 / ior2 as closest_hit.cu:496-498 */
} skh_bsdf_query;
typedef struct skh_bsdf_result
{
    float k2[3], bsdf_over_pdf[3], pdf; /* Bsdf_sample_data */
    int32_t event_type; /* mi::neuraylib::Bsdf_event_type bits */
    float bsdf_diffuse[3], bsdf_glossy[3], eval_pdf; /* Bsdf_evaluate_data: both include the cosine */
    uint32_t reserved0;
} skh_bsdf_result;
skh_status skh_bsdf_probe(skh_context* ctx, const skh_bsdf_query* queries, uint32_t n, skh_bsdf_result* results);

/* ---- unit probes (tests) ----
 * The device functions of the sampler (A2), the light samplers / pdfs / MIS weight (A4, A5) and the accumulator (A10), run on the GPU
 * one call per record, so that GPU tests can hold the HIP code against the fixtures the REFERENCE's own headers produced
 * (tests/golden/, generated by oracle/ref_golden.cpp).  Reference code probed: RandomSampler.h:130-137,166-175,213-226;
 * Lights.h:28-84,201-362; OptixRender.cu:60-78 + postprocessing/Utils.h:5-14.  Records are packed 32-bit words:
 *   unit                    consts               in (per record)                          param                         out (per record)
 *   SKH_UNIT_SAMPLER        --                   u32 x, y, sampleIndex, depth, dim        sppTotal                      u32 bits of random<dim>, bits of the same
 *                                                                                                                       value through the LDS-table path k_shade uses, sampleIdx
 *   SKH_UNIT_SOBOL          --                   u32 index, dim                           --                            u32 sobol_uint
 *   SKH_UNIT_LIGHT_SAMPLE   UniformLight (112 B) f32 P[3], u[2]                           0 rect uniform | 1 spherical  f32 pointOnLight[3], pdf, normal[3], area,
 *                                                                                         rect | 2 sphere | 3 distant   L[3], distToLight
 *   SKH_UNIT_LIGHT_PDF      UniformLight         f32 lightHitPoint[3], surfacePoint[3]    --                            f32 getLightPdf
 *   SKH_UNIT_LIGHT_NORMAL   UniformLight         f32 hitPoint[3]                          --                            f32 calcLightNormal[3], calcLightArea
 *   SKH_UNIT_MIS            --                   f32 a, b                                 --                            f32 misWeightBalance(a, b)
 *   SKH_UNIT_ACCUMULATE     f32 exposure[3]      f32 value[3]  (a SEQUENCE: record k is   first sub-frame index         f32 accumulator[3] after record k
 *                                                folded into the result of 0..k-1)
 *   SKH_UNIT_TONEMAP        f32 exposure[3]      f32 color[3]                             --                            f32 tonemap[3], inverseTonemap[3]
 *   SKH_UNIT_LIBM           --                   f32 x, y                                 --                            f32 sin x, cos x, acos x, asin x, atan2(y, x), exp x, log x,
 *                                                                                                                       sinh x, pow(x, y), atan2(x, y): strelka_amd/csrc/skh_libm.h,
 *                                                                                                                       the libm stand-ins both sides compile
 *   SKH_UNIT_ENV_SAMPLE     --                   f32 u[2] (row, column)                   --                            f32 dir[3], pdf, Le[3], u32 ix, iy (the texel selected)
 *   SKH_UNIT_ENV_EVAL       --                   f32 dir[3]                               --                            f32 Le[3], pdf, u32 ix, iy
 *   (both on the context's current environment, skh_set_environment below; pdf and Le are those of the returned direction) */
typedef enum skh_unit
{
    SKH_UNIT_SAMPLER = 0,
    SKH_UNIT_SOBOL = 1,
    SKH_UNIT_LIGHT_SAMPLE = 2,
    SKH_UNIT_LIGHT_PDF = 3,
    SKH_UNIT_LIGHT_NORMAL = 4,
    SKH_UNIT_MIS = 5,
    SKH_UNIT_ACCUMULATE = 6,
    SKH_UNIT_TONEMAP = 7,
    SKH_UNIT_LIBM = 8,
    SKH_UNIT_ENV_SAMPLE = 9,
    SKH_UNIT_ENV_EVAL = 10,
    SKH_UNIT_COUNT = 11
} skh_unit;
skh_status skh_unit_probe(skh_context* ctx, uint32_t unit, uint32_t param, const void* consts, const void* in, uint32_t n, void* out);

/* ---- options / stats ----
 * None of the options changes a result: hit records and images are bit-identical for every setting
 * (tests/test_gpu_parity.py::test_results_do_not_depend_on_the_acceleration_structure_or_scheduling) -- with ONE exception,
 * bake_world, which is part of the intersection's definition: a baked instance's triangles are tested in world space, so the
 * t, u, v of hits on it differ in the last bits from the object-space test (same instance, same primitive; the CPU oracle
 * takes the same setting and the bit-exact contract holds per setting).
 *   measurement   count_traversal 0|1 (counter build of the trace kernels), timing 0|1 (per-kernel hipEvent spans)
 *   scheduling    waves_per_cu (28) / waves_per_cu_shadow (28) (7 waves per SIMD) / waves_per_cu_world, waves_per_cu_shadow_world (32 / 32: the world-only builds run 8), fetch_min_closest / fetch_min_shadow (32 / 48, scenes with curves 16 / 16: idle lanes before a wave refills), fetch_min_closest_small (48: the closest-hit threshold of small overlapped passes of triangle scenes, unless fetch_min_closest is set),
 *                 merge_light_proxies (0; 1: baked light proxies share the baked mesh triangles' world-space tree and any-hit queries skip their triangles -- closest-hit -2 ... -4 %, any-hit +8 ... +13 %: measured a net loss; 0: a tree of their own, visited by the radiance rays that meet the box around all of them),
 *                 compact_hits (1: render passes of scenes the world-only kernels trace, whose instance count and primitive range share 32 bits, keep 16-byte hit records {t, u, v, instance | record or segment}; 0: 32-byte records always),
 *                 direct_records (-1 = by the counts: a baked mesh triangle's hit names its shading record, unless only (instance, mesh-local primitive) fits a 16-byte hit record; 0 / 1 forced),
 *                 fetch_chunk (-1 = auto: 128 when the triangle + curve trees hold <= 16384 nodes, else 0; queue positions a trace wave reserves per atomic on its shard's cursor),
 *                 queue_order (1: a pass of several sub-frames queues its camera rays cell by cell, all sub-frames of a cell together, the cells dealt round-robin to the
 *                 queue's shards along a Morton curve over the tiles; 0: in slot order, sub-frame after sub-frame.  A one-sub-frame pass is the same under both),
 *                 cell_blocks (0 = auto: -1; -1: a cell is one 64-slot chunk, an 8 x 8 pixel block; n >= 1: n 512-slot blocks, 2 = a 32 x 32 tile),
 *                 node_break_closest / node_break_shadow (32 / 28, curves 20 / 20 until one is set explicitly: leave the node loop below x/64 descending rays),
 *                 leaf_min (16: lanes for the minority kind of leaf work), curve_min (48: lanes parked in front of the
 *                 curve intersector before it runs), subframe_batch (0 = auto: ~64 M paths per pass), aov_band (2^22; 64 ... 2^26: rays per band of skh_render_aovs),
 *                 speculate (8: sub-frames traced ahead when skh_render_subframe is called once per sub-frame; 0 = off),
 *                 speculate_async 1|0 (the pass after the one being collected is traced meanwhile, on the render stream, into a second
 *                 path-state buffer; accumulation steps and skh_buffer_download run beside it on their own stream: the caller's map()
 *                 copies cost nothing any more.  A camera move waits for the pass in flight, <= `speculate` sub-frames),
 *                 overlap 0|1|2 (any-hit launches on a second stream beside the next closest-hit launch: off | small passes |
 *                 always), small_waves_closest / small_waves_shadow (shares of a 32-wave CU the two overlapped launches of a small pass take, scaled to what their build fits; 0 = automatic: 20 / 12 for triangle scenes -- the closest-hit launch is the one on the critical path --, 16 / 16 with curves; >= 32 = the full grid), small_waves_first / small_waves_last (the same for the pass's FIRST closest-hit and LAST any-hit launch, which run alone; 0 = automatic: as the others, the last any-hit launch of a triangle scene 20),
 *                 tail_split (1 | 2 | 0 | -1: the world-only triangle kernels' build whose waves, once the ray queue is dry, hand stack entries of their last rays to their idle lanes -- a long ray's
 *                 subtrees walked side by side, results merged by the closest-hit rule: same records --; 1 = every launch of a scene whose hierarchy has more than 16 384 nodes, the default; 2 = every launch; -1 = passes of
 *                 2^17 ... 2^23 paths only; 0 = never)
 *   definition    bake_world 4|3|2|1|0 (mesh instances intersected in world space, no instance entry: 1 = instances whose mesh has one
 *                 user -- what HdStrelka's per-instance meshes are --, 2 = also instances of meshes with <= bake_small_tris (64)
 *                 triangles when that empties the top level, 3 = every mesh instance, 4 (default) = 3 while the instanced triangles stay
 *                 within bake_budget_mtris (64) million, else 2; 0 = every instance keeps its TLAS leaf), world_kernel 1|0 (scenes
 *                 with an empty top level run the world-only build of the traversal kernel; curve instances -- at most 16, no unbaked
 *                 mesh or light instance beside them -- do not need a top level either: their trees are walked from the world-only kernel with the
 *                 curve block, each instance's transform applied to the ray as at a TLAS leaf),
 *                 env_nee 1|0 (the second option that is part of a definition, the estimator's: 1 = the environment is an entry of the light pick and a miss is
 *                 MIS-weighted against it; 0 = the environment is reached by BSDF sampling only, every miss weighs 1.  Two estimators of one integral: the
 *                 expectation is the same, the bits are not.  Without an environment it changes nothing),
 *                 emit_nee 1|0 (the same for emissive meshes: 1 = the emitter set is an entry of the light pick and a hit on an emitter is MIS-weighted against it; 0 = never
 *                 picked, every emitter hit weighs 1.  Same expectation, other bits; with no emissive material it changes nothing),
 *                 cutout_rounds (8; 1..32: rejected hits per ray before the next hit is accepted whatever its opacity -- skh_set_material_cutouts; values outside the range
 *                 are refused.  Without a cutout in use it changes nothing)
 *   build        build_quality 1|0 (PLOC | Karras radix tree), reinsert_rounds (8; 0 = off: rounds of parallel reinsertion over the PLOC tree of the
 *                 triangle build -- every subtree looks for the place in the tree where it costs least, the best non-conflicting moves are applied),
 *                 reinsert_curve_rounds (4: the same over the curve sub-segment trees),
 *                 reinsert_min_size (0 = auto: 1 up to 4 M triangles, 32 beyond: only the part of the tree above subtrees of this many primitives is optimised), morton_bits (10 per axis in the sort keys; 4..21), ploc_top (0: clusters left at which the triangle build widens PLOC's neighbour search from 12 to 96), leaf_max_tris (2), leaf_lines 0|1 (triangle leaves padded so that none
 *                 straddles a 128-byte line it need not: -11 % fetched lines, same time, more memory), curve_leaf (1), curve_split (4: parameter sub-ranges
 *                 per curve segment), tlas_build 1|0|2 (GPU PLOC over the instance boxes (default) | exact sweep SAH on the host: 5 % fewer instance
 *                 entries, single-threaded | the sweep up to 8192 instances, the GPU beyond), tlas_open (1: TLAS leaves per instance budget),
 *                 tight_instance_boxes 1|0
 *   (round 4's `wide` 8, `tail_park`, `tail_lag` are gone: measured negatives, experiments/README.md)
 * Unknown names and out-of-range values return SKH_INVALID_ARGUMENT. */
skh_status skh_set_option(skh_context* ctx, const char* name, int64_t value);
/* what the context's device reports (hipDeviceProp_t): the measurement code prices instruction rates against these */
typedef struct skh_device_info
{
    uint32_t compute_units; /* 256 on MI355X */
    uint32_t simds_per_cu; /* 4 */
    uint32_t clock_khz; /* maximum engine clock */
    uint32_t memory_clock_khz;
    uint32_t memory_bus_bits;
    uint32_t wavefront_size;
    uint64_t total_memory_bytes;
    char name[64];
} skh_device_info;
skh_status skh_get_device_info(skh_context* ctx, skh_device_info* out);
/* what the last skh_build_accel did to the triangle hierarchy (the builder that replaces optixAccelBuild with PREFER_FAST_TRACE,
 * OptixRender.cpp:318-386): PLOC over the Morton order, then rounds of parallel reinsertion (options reinsert_rounds / reinsert_min_size) */
typedef struct skh_build_info
{
    uint32_t triangles; /* primitives of the triangle build (meshes + baked world-space groups) */
    uint32_t nodes; /* 64-byte 4-wide nodes */
    uint32_t reinsert_rounds; /* rounds that ran (a round without a move ends the pass) */
    uint32_t reinsert_moves; /* subtrees moved, all rounds */
    uint32_t reinsert_min_size; /* truncation used: only nodes whose parent holds at least this many primitives moved */
    uint32_t refit; /* 1: the hierarchy in use came out of skh_refit_accel's refit (topology of the last build, boxes of the current vertices); 2: out of skh_update_accel's
                       in-place update, top level included (topology of the last build, boxes of the current transforms, vertices and control points); 0: out of a build */
    double cost_before; /* sum of the internal binary nodes' box half-areas after PLOC ... */
    double cost_after; /* ... and after the reinsertion pass (== cost_before when it did not run) */
    double ms_reinsert; /* wall time of the pass, inside ms_build */
    double ms_build; /* == skh_stats.ms_build */
    double ms_refit; /* wall time of the last refit or in-place update (leaf records gathered again + one launch per tree level + the shading tables) */
} skh_build_info;
skh_status skh_get_build_info(skh_context* ctx, skh_build_info* out);
skh_status skh_get_stats(skh_context* ctx, skh_stats* out);
skh_status skh_reset_stats(skh_context* ctx);
skh_status skh_synchronize(skh_context* ctx);
void* skh_get_stream(skh_context* ctx); /* hipStream_t the kernels are launched on */

#ifdef __cplusplus
}
#endif
#endif /* STRELKA_HIP_H */
