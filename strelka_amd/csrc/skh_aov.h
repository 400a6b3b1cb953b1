// skh_aov.h -- the first-hit AOV pass (skh_render_aovs; include/strelka_hip.h and DESIGN.md section 2 "First-hit AOVs" are the definition).
//
//   k_aov_raygen   one camera ray per pixel of a band of the region -> skh_ray records, region order
//   (the trace)    skh_trace_device's internal path on those records, closest-hit: cutouts, blending under the raw rule and cutout_rounds come with it
//   k_aov_resolve  the 20-byte skh_hit of every pixel -> one 16-byte word group per requested plane
//
// The ray is k_raygen's (generate_camera_ray, sampler_random), the surface state k_shade's (fill_triangle / fill_curve, resolve_material, tex_lookup_rgba8):
// the same functions, called here, so that the planes and the renderer cannot drift apart.  No LDS, no atomics; the plane mask is uniform per launch.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_kernels.h"

namespace skh
{

struct AovP // by-value kernel argument: skh_aov_params + the context's image size + where the band lies in the region
{
    float viewToWorld[16];
    float clipToView[16];
    float worldToClip[16];
    uint32_t imageW, imageH; // skh_resize's
    uint32_t x0, y0, width;  // the region
    uint32_t first, count;   // the band: region pixels [first, first + count)
    uint32_t sampleIndex, sppTotal;
    float tmin;
};

__global__ void __launch_bounds__(256) k_aov_raygen(AovP ap, float4* __restrict__ rays /* skh_ray: two float4 per ray */)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ap.count)
        return;
    const uint32_t g = ap.first + i;
    const uint32_t ry = g / ap.width;
    const uint32_t px = ap.x0 + (g - ry * ap.width), py = ap.y0 + ry;
    float jx = 0.5f, jy = 0.5f;
    if (ap.sampleIndex != SKH_AOV_PIXEL_CENTRE)
    {
        const Sampler s = init_sampler(px, py, ap.sampleIndex, ap.sppTotal, 52u); // k_raygen's sampler for that sample
        jx = sampler_random(s, DIM_PIXEL_X), jy = sampler_random(s, DIM_PIXEL_Y);
    }
    v3 o, d;
    generate_camera_ray(px, py, ap.imageW, ap.imageH, ap.clipToView, ap.viewToWorld, jx, jy, o, d);
    rays[2 * (size_t)i] = make_float4(o.x, o.y, o.z, ap.tmin);
    rays[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, 1e16f);
}

#define SKH_AOV_BIT(k) (1u << (k))
// the planes that need the surface state of the hit (everything but the ids and the hit's own t, u, v)
#define SKH_AOV_SURFACE_BITS (SKH_AOV_BIT(SKH_AOV_NORMAL) | SKH_AOV_BIT(SKH_AOV_POSITION) | SKH_AOV_BIT(SKH_AOV_GEOM_NORMAL) | SKH_AOV_BIT(SKH_AOV_ALBEDO) | SKH_AOV_BIT(SKH_AOV_TEXCOORD))

SKH_DI uint4 f4(float x, float y, float z, float w)
{
    return make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), __float_as_uint(w));
}

struct AovPlanes // by-value kernel argument: plane k of the caller, already offset to the band's first pixel (nullptr: not asked for)
{
    uint4* p[SKH_AOV_COUNT];
};

__global__ void __launch_bounds__(256) k_aov_resolve(DevScene sc, MtexP mtex, AovP ap, uint32_t planes, const float4* __restrict__ rays,
                                                      const skh_hit* __restrict__ hits, AovPlanes out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ap.count)
        return;
    const bool wantIds = (planes & SKH_AOV_BIT(SKH_AOV_IDS)) != 0u, wantHit = (planes & SKH_AOV_BIT(SKH_AOV_HIT)) != 0u;
    const bool wantN = (planes & SKH_AOV_BIT(SKH_AOV_NORMAL)) != 0u, wantP = (planes & SKH_AOV_BIT(SKH_AOV_POSITION)) != 0u;
    const bool wantNg = (planes & SKH_AOV_BIT(SKH_AOV_GEOM_NORMAL)) != 0u, wantAlbedo = (planes & SKH_AOV_BIT(SKH_AOV_ALBEDO)) != 0u;
    const bool wantUv = (planes & SKH_AOV_BIT(SKH_AOV_TEXCOORD)) != 0u;
    // (the depth word is a function of the position)
    const bool wantSurface = (planes & SKH_AOV_SURFACE_BITS) != 0u || wantHit;

    const skh_hit h = hits[i];
    const bool miss = h.instance_id == 0xffffffffu;
    uint32_t kind = 0u, material = 0xffffffffu;
    float facing = 0.0f, depth = 1.0f, tu = 0.0f, tv = 0.0f;
    v3 P = mk3(0.0f), N = mk3(0.0f), Ng = mk3(0.0f);
    v4 albedo = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    float pw = 0.0f;
    if (!miss)
    {
        const HostInstance hi = sc.instances[h.instance_id];
        kind = hi.type == 0u ? 1u : (hi.type == 2u ? 2u : 3u);
        if (kind != 3u)
        {
            const uint32_t mid0 = hi.material == 0xffffffffu ? 0u : hi.material; // k_shade's index
            material = mid0 < sc.numMaterials ? mid0 : 0u;
        }
        if (wantSurface)
        {
            const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
            const v3 rayO = mk3(r0), rayD = mk3(r1);
            pw = 1.0f;
            if (kind == 3u)
            {
                P = rayO + h.t * rayD;
                albedo = mk4(1.0f, 1.0f, 1.0f, 1.0f);
            }
            else
            {
                const float* w2o = sc.inst[h.instance_id].w2o;
                const bool wantMat = wantAlbedo || wantN; // (the normal map's id is the material's)
                Material mat;
                if (wantMat)
                    mat = sc.materials[material];
                if (kind == 1u)
                {
                    // the triangle's shading record: three float4 for the geometry, two more only where a texture coordinate is read
                    const bool wantTex = wantUv || (wantMat && sc.numTextures != 0u);
                    const float4* tp = sc.shadeTris + 6 * (size_t)(hi.light + h.prim_id);
                    float4 tri[3], tx[2];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        tri[k] = tp[k];
                    tx[0] = tx[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (wantTex)
                        tx[0] = tp[3], tx[1] = tp[4];
                    SurfaceTex st;
                    st.u = st.v = 0.0f, st.tangent_u = st.tangent_v = mk3(0.0f);
                    // (two calls, not one with a selected pointer: `st` then stays in registers)
                    const SurfaceHit sh = wantTex ? fill_triangle(hi, w2o, tri, tx, h.u, h.v, false, &st) : fill_triangle(hi, w2o, tri, tx, h.u, h.v, false, nullptr);
                    P = sh.position, N = sh.normal, Ng = sh.geom_normal;
                    tu = st.u, tv = st.v;
                    if (wantN && mtex_valid(mat.normal_texture, sc.numTextures))
                    {
                        // k_shade's normal map: base::tangent_space_normal_texture, factor 1
                        const v4 c = tex_lookup_rgba8(sc.texels, sc.texDesc[mat.normal_texture - 1u], st.u, st.v);
                        const v3 ts = mk3(c.x * 2.0f - 1.0f, c.y * 2.0f - 1.0f, c.z * 2.0f - 1.0f);
                        N = normalize((st.tangent_u * ts.x + st.tangent_v * ts.y) + sh.normal * ts.z);
                    }
                    if (wantAlbedo)
                    {
                        v3 Le = mk3(0.0f); // (no emission look-up: the base colour does not depend on it)
                        resolve_material(sc.texels, sc.texDesc, sc.numTextures, mat, mtex_entry(mtex, material), Le, st.u, st.v);
                    }
                }
                else
                {
                    const SurfaceHit sh = fill_curve(sc, hi, w2o, h.prim_id, h.u, h.t, rayO, rayD, false, nullptr);
                    P = sh.position, N = sh.normal, Ng = sh.normal;
                }
                facing = dot(Ng, -rayD) >= 0.0f ? 1.0f : -1.0f; // (a curve's too: its Ng is its N)
                if (wantAlbedo)
                    albedo = mk4(mat.base_color[0], mat.base_color[1], mat.base_color[2], 1.0f);
            }
            if (wantHit)
            {
                const v4 clip = mul44(ap.worldToClip, mk4(P.x, P.y, P.z, 1.0f));
                depth = clip.z / clip.w;
            }
        }
    }
    if (wantIds)
        out.p[SKH_AOV_IDS][i] = make_uint4(miss ? 0xffffffffu : h.instance_id, miss ? 0xffffffffu : h.prim_id, material, kind);
    if (wantHit)
        out.p[SKH_AOV_HIT][i] = miss ? f4(-1.0f, 0.0f, 0.0f, 1.0f) : f4(h.t, h.u, h.v, depth);
    if (wantN)
        out.p[SKH_AOV_NORMAL][i] = f4(N.x, N.y, N.z, facing);
    if (wantP)
        out.p[SKH_AOV_POSITION][i] = f4(P.x, P.y, P.z, pw);
    if (wantNg)
        out.p[SKH_AOV_GEOM_NORMAL][i] = f4(Ng.x, Ng.y, Ng.z, 0.0f);
    if (wantAlbedo)
        out.p[SKH_AOV_ALBEDO][i] = f4(albedo.x, albedo.y, albedo.z, albedo.w);
    if (wantUv)
        out.p[SKH_AOV_TEXCOORD][i] = f4(tu, tv, 0.0f, 0.0f);
}

} // namespace skh
