// strelka_hip -- the body of k_shade (skh_kernels.h), compiled twice: into k_shade (LSHAPE = false) and into k_shade_lshape (LSHAPE = true, with `lsh`).
// Included inside the kernel's braces: it sees the kernel's arguments and template flags HAIR, ENV, EMIT, MTEX, POS and the constant LSHAPE.
    // the bounce's position (skh_kernels.h): `depth == 0` and "no path goes on from here" as constants of the build
    constexpr bool kLast = POS == SHADE_LAST;
    const bool depth0 = POS == SHADE_ANY ? depth == 0u : POS == SHADE_FIRST;
    // the path-state loads of a MIDDLE build stay behind the (always true) runtime test they were behind: as straight-line code the scheduler hoists them over the
    // hit record's and the build spills 8 registers at five waves
    const bool stateInit = POS == SHADE_MIDDLE ? depth == 0u : depth0;
    // entries of the light pick: the lights, behind them the environment when it is sampled (option env_nee), behind that the emitter set (option emit_nee)
    const uint32_t numPick = (ENV ? sc.numLights + (env.nee ? 1u : 0u) : sc.numLights) + (EMIT ? (emit.nee ? 1u : 0u) : 0u);
    __shared__ uint32_t s_wave[2 * (SKH_COMPACT_MAX_WAVES + 1)];
    __shared__ uint32_t s_sobol[SKH_SOBOL_LUT_WORDS];
#if SKH_MATERIALS_LDS
    // north_star: "material params staged through LDS": the first SKH_MATERIALS_LDS argument blocks (64 B each) ride along with the
    // Sobol table; a hit whose material lies beyond them reads global memory as before
    __shared__ float4 s_mat[SKH_MATERIALS_LDS * 4];
#endif
    // workgroup b works on shard b & 7 (and compacts into the same shard of both output queues)
    const uint32_t shard = blockIdx.x & (SKH_SHARDS - 1u), lb = blockIdx.x / SKH_SHARDS;
    const uint32_t n = countPtr[shard * SKH_COUNT_STRIDE]; // rays in this shard
    if (lb * blockDim.x >= n)
        return; // whole block past the end of its shard
    const uint32_t il = lb * blockDim.x + threadIdx.x;
    const uint32_t i = shard * rq.region + il;
#ifdef SKH_LANE_PROFILE
    unsigned long long spc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, spT = __builtin_readcyclecounter();
#define SKH_SP(k)                                                    \
    {                                                                \
        const unsigned long long t_ = __builtin_readcyclecounter();  \
        spc[k] += t_ - spT;                                          \
        spT = t_;                                                    \
    }
#else
#define SKH_SP(k)
#endif
    bool valid = il < n;
    uint32_t pid = 0;
    v3 rayO = mk3(0.0f), rayD = mk3(0.0f);
    float4 hr0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hr1 = hr0;
    {
        // 20 KB table -> LDS: the block's five fetches go out together (a rolled loop waited for each in turn)
        constexpr int passes = ((SKH_SOBOL_LUT_WORDS / 4) + SKH_SHADE_BLOCK - 1) / SKH_SHADE_BLOCK; // (256 threads: five whole passes; 512: the third is half one)
        uint4 lut[passes];
#pragma unroll
        for (int k = 0; k < passes; ++k)
            if ((k + 1) * SKH_SHADE_BLOCK <= SKH_SOBOL_LUT_WORDS / 4 || threadIdx.x + k * SKH_SHADE_BLOCK < SKH_SOBOL_LUT_WORDS / 4)
                lut[k] = reinterpret_cast<const uint4*>(g_sobol_lut)[threadIdx.x + k * SKH_SHADE_BLOCK];
            else
                lut[k] = make_uint4(0u, 0u, 0u, 0u);
#if SKH_MATERIALS_LDS
        float4 mrow = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        static_assert(SKH_MATERIALS_LDS * 4 <= SKH_SHADE_BLOCK, "one float4 of the material table per thread");
        if (threadIdx.x < SKH_MATERIALS_LDS * 4 && threadIdx.x < sc.numMaterials * 4u)
            mrow = reinterpret_cast<const float4*>(sc.materials)[threadIdx.x];
#endif
#pragma unroll
        for (int k = 0; k < passes; ++k)
            if ((k + 1) * SKH_SHADE_BLOCK <= SKH_SOBOL_LUT_WORDS / 4 || threadIdx.x + k * SKH_SHADE_BLOCK < SKH_SOBOL_LUT_WORDS / 4)
                reinterpret_cast<uint4*>(s_sobol)[threadIdx.x + k * SKH_SHADE_BLOCK] = lut[k];
#if SKH_MATERIALS_LDS
        if (threadIdx.x < SKH_MATERIALS_LDS * 4)
            s_mat[threadIdx.x] = mrow;
#endif
    }
    __syncthreads();
    bool emitNext = false, emitShadow = false;
    v3 nextO = mk3(0.0f), nextD = mk3(0.0f), shO = mk3(0.0f), shD = mk3(0.0f), shC = mk3(0.0f);
    float shTmax = 0.0f;
    if (valid)
    {
        pid = rq.ids()[i];
        rayO = mk3(rq.plane(0)[i], rq.plane(1)[i], rq.plane(2)[i]);
        rayD = mk3(rq.plane(3)[i], rq.plane(4)[i], rq.plane(5)[i]);
        if (hq.primBits != 0u)
        {
            // the 16-byte record of a world-only triangle scene: every mesh hit there names its shading record (SKH_PRIM_DIRECT); a light proxy's
            // primitive index is not looked at by its hit program
            hr0 = *hq.rec16(i);
            const uint32_t w = __float_as_uint(hr0.w);
            hr1.x = __uint_as_float(w == 0xffffffffu ? w : w >> hq.primBits);
            hr1.y = __uint_as_float(w == 0xffffffffu ? w : ((w & ((1u << hq.primBits) - 1u)) | (hq.direct ? SKH_PRIM_DIRECT : 0u)));
        }
        else
            hr0 = hq.rec(i)[0], hr1 = hq.rec(i)[1];
        const float ht = hr0.x, hu = hr0.y, hv = hr0.z;
        const uint32_t hinst = __float_as_uint(hr1.x), hprim = __float_as_uint(hr1.y);
        float* P = ps.base;
        const size_t S = ps.stride;
        // (depth 0: the PerRayData initial values, OptixRender.cu:96-109 -- k_raygen does not store them)
        v3 throughput = stateInit ? mk3(1.0f) : mk3(P[pid], P[pid + S], P[pid + 2 * S]);
        // prd.radiance stays in the path state and is read-modify-written only by the branches that change it (a light hit, the debug and error
        // colours; the miss program's `+= throughput * 0` only when that product is not zero, i.e. a non-finite throughput): most paths of most
        // bounces leave it alone, and 12 B read + 12 B written per path were a tenth of this kernel's traffic.  Same values in the same order.
        v3 radiance = mk3(0.0f);
        bool radianceDirty = false;
#define SKH_RADIANCE_LOAD() radiance = mk3(ps.rad()[pid]), radianceDirty = true
        float lastBsdfPdf = stateInit ? 0.0f : P[pid + 6 * S];
        uint32_t flags = stateInit ? 0u : reinterpret_cast<uint32_t*>(P)[pid + 7 * S];
        bool inside = (flags & PF_INSIDE) != 0;
        bool specularBounce = (flags & PF_SPECULAR) != 0;
        uint32_t firstEvent = (flags >> PF_EVENT_SHIFT) & 3u;
        uint32_t px, py;
        const uint32_t sub = pid / fp.numSlots;
        slot_to_pixel(fp, tileXY, pid - sub * fp.numSlots, px, py);
        Sampler smp = init_sampler(px, py, fp.subframeIndex + sampleOffset + sub, fp.sppTotal, 52u);
        smp.depth = POS == SHADE_FIRST ? 0u : depth; // prd.sampler.depth++ once per bounce (OptixRender.cu:153)
        uint32_t prdDepth = smp.depth;
        v3 origin = rayO, dir = rayD; // prd.origin / prd.dir keep their old value when no hit program sets them

        if (hinst == 0xffffffffu)
        {
            if constexpr (ENV)
            {
                // the environment seen by a ray that leaves the scene: weighted as __closesthit__light weighs a light it hits
                const EnvEval ee = env_eval(env, rayD);
                SKH_RADIANCE_LOAD();
                if (depth0 || specularBounce || !env.nee)
                    radiance = radiance + throughput * ee.Le;
                else
                {
                    const float lightPdf = ee.pdf / (float)numPick;
                    const float misWeight = mis_weight_balance(lastBsdfPdf, lightPdf);
                    radiance = radiance + throughput * ee.Le * misWeight;
                }
            }
            else
            {
                // __miss__ms: bg_color = 0 (OptixRender.cpp:739)
                const v3 bg = throughput * mk3(0.0f);
                if (!(bg.x == 0.0f && bg.y == 0.0f && bg.z == 0.0f))
                {
                    SKH_RADIANCE_LOAD();
                    radiance = radiance + bg;
                }
            }
            throughput = mk3(0.0f);
            prdDepth = fp.maxDepth;
        }
        else
        {
            SKH_SP(0) // queue / path-state loads, sampler
            const HostInstance hi = sc.instances[hinst];
            const float* w2o = sc.inst[hinst].w2o;
            // A hit on a baked triangle names its shading record itself (SKH_PRIM_DIRECT, k_gather_tris): the 96-byte fetch -- the one that
            // misses the caches -- goes out BESIDE the instance record's instead of behind it (chain: queue -> {instance, triangle} -> material,
            // was queue -> instance -> {triangle, material}).  Other hits read record 0 here for nothing and theirs below.
            const bool directTv = (hprim & SKH_PRIM_DIRECT) != 0u;
            float4 tv[3], tx[2];
            // (tangents / UVs: only a textured material or a hair material on a mesh reads them -- scenes without either do not fetch them)
            const bool txWanted = HAIR || sc.numTextures != 0u;
            tx[0] = tx[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            {
                // (a 16-byte record -- HitQ::primBits -- marks every hit as direct: a curve segment's index must not leave the table)
                const uint32_t recIdx = directTv ? (hprim & ~SKH_PRIM_DIRECT) : 0u;
                const float4* tp = sc.shadeTris + 6 * (size_t)(hq.primBits ? min(recIdx, hq.recClamp) : recIdx);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    tv[k] = tp[k];
                if (txWanted)
                    tx[0] = tp[3], tx[1] = tp[4];
            }
            // (the whole record now: the compiler sinks the loads of `material` / `light` below the type test = one more round trip)
            asm volatile("" ::"v"(hi.type), "v"(hi.material), "v"(hi.light));
            if (hi.type == 1)
            {
                // __closesthit__light
                const uint32_t lidx = hi.light < sc.numLights ? hi.light : 0u; // (skh_build_accel validates it; the light list may have been replaced since)
                const Light& l = sc.lights[lidx];
                const v3 hitPoint = rayO + ht * rayD;
                if constexpr (LSHAPE)
                {
                    // the proxy of a shaped light: a sampled disk answers with its unit normal and weighs the hit against the sampler's pdf; a cone scales
                    // the radiance by s(dot(axis, -rayD)), at depth 0 and after a specular bounce too
                    const Lshape lse = lshape_fetch(lsh, lidx); // (beside the light's record)
                    const bool sampledDisc = l.type == 1 && (lse.flags & SKH_LSHAPE_SAMPLE_DISC) != 0u;
                    const v3 lightNormal = sampledDisc ? normalize(mk3(l.normal)) : calc_light_normal(l, hitPoint);
                    if (-dot(rayD, lightNormal) > 0.0f)
                    {
                        const v3 Li = mk3(l.color) * lshape_cone(lse, -rayD);
                        SKH_RADIANCE_LOAD();
                        if (depth0 || specularBounce)
                            radiance = radiance + throughput * Li * -dot(rayD, lightNormal);
                        else
                        {
                            const float lightPdf = (sampledDisc ? disc_light_pdf(l, hitPoint, rayO) : get_light_pdf(l, hitPoint, rayO)) / (float)numPick;
                            const float misWeight = mis_weight_balance(lastBsdfPdf, lightPdf);
                            radiance = radiance + throughput * Li * -dot(rayD, lightNormal) * misWeight;
                        }
                    }
                }
                else
                {
                    const v3 lightNormal = calc_light_normal(l, hitPoint);
                    if (-dot(rayD, lightNormal) > 0.0f)
                    {
                        SKH_RADIANCE_LOAD();
                        if (depth0 || specularBounce)
                            radiance = radiance + throughput * mk3(l.color) * -dot(rayD, lightNormal);
                        else
                        {
                            const float lightPdf = get_light_pdf(l, hitPoint, rayO) / (float)numPick;
                            const float misWeight = mis_weight_balance(lastBsdfPdf, lightPdf);
                            radiance = radiance + throughput * mk3(l.color) * -dot(rayD, lightNormal) * misWeight;
                        }
                    }
                }
                throughput = mk3(0.0f);
            }
            else
            {
                // __closesthit__radiance
                const uint32_t mid = hi.material == 0xffffffffu ? 0u : hi.material; // OptixRender.cpp:768
                float4 matLe = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if constexpr (EMIT) // (beside the material's record: one round trip for both)
                    matLe = emit.Le[mid < emit.numMaterials ? mid : 0u];
                MtexEntry mte;
                if constexpr (MTEX) // (likewise)
                    mte = mtex_entry(mtex, mid < sc.numMaterials ? mid : 0u);
#if SKH_MATERIALS_LDS
                const uint32_t midc = mid < sc.numMaterials ? mid : 0u;
                Material mat;
                if (midc < (uint32_t)SKH_MATERIALS_LDS)
                {
                    const float4 m0 = s_mat[4 * midc], m1 = s_mat[4 * midc + 1], m2 = s_mat[4 * midc + 2], m3 = s_mat[4 * midc + 3];
                    mat.type = __float_as_uint(m0.x), mat.base_color[0] = m0.y, mat.base_color[1] = m0.z, mat.base_color[2] = m0.w;
                    mat.roughness = m1.x, mat.metallic = m1.y, mat.specular = m1.z, mat.ior = m1.w;
                    mat.base_color_texture = __float_as_uint(m2.x), mat.normal_texture = __float_as_uint(m2.y);
                    mat.reserved[0] = m2.z, mat.reserved[1] = m2.w, mat.reserved[2] = m3.x, mat.reserved[3] = m3.y, mat.reserved[4] = m3.z, mat.reserved[5] = m3.w;
                }
                else
                    mat = sc.materials[midc];
#else
                Material mat = sc.materials[mid < sc.numMaterials ? mid : 0u];
#endif
                // the triangle's shading record goes out together with the material's (both hang off the instance record only);
                // a curve hit fetches record 0 for nothing
                if (!directTv && hi.type != 2)
                {
                    const float4* tp = sc.shadeTris + 6 * (size_t)(hi.light + hprim);
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        tv[k] = tp[k];
                    if (txWanted)
                        tx[0] = tp[3], tx[1] = tp[4];
                }
                asm volatile("" ::"v"(mat.type), "v"(tv[0].x), "v"(tv[1].x), "v"(tv[2].x));
                // mdlcode_init (closest_hit.cu:507): texture lookups of the material, triangle hits only.  OmniPBR: a valid
                // diffuse_texture replaces the constant colour; a valid normalmap_texture replaces state.normal by
                // normalize(tu x + tv y + n z), (x, y, z) = 2 rgb - 1 (base::tangent_space_normal_texture, factor 1)
                const bool useBase = mat.base_color_texture != 0u && mat.base_color_texture <= sc.numTextures;
                const bool useNormal = mat.normal_texture != 0u && mat.normal_texture <= sc.numTextures;
                bool mtexWanted = false;
                if constexpr (MTEX)
                    mtexWanted = mtex_wanted(mat, mte, sc.numTextures, matLe.w > 0.0f);
                const bool textured = hi.type != 2 && (useBase || useNormal || mtexWanted);
                SurfaceTex st;
                v3 stT = mk3(0.0f);
                // (a hair material on a triangle mesh reads state.tangent_u too: the vertex tangent, closest_hit.cu:399-400)
                const bool hairOnMesh = HAIR && mat.type == 3u && hi.type != 2;
                SurfaceHit sh = hi.type == 2 ? fill_curve(sc, hi, w2o, hprim & ~SKH_PRIM_DIRECT /* (a segment index never has the bit; a 16-byte record sets it for every hit) */, hu, ht, rayO, rayD, inside, HAIR ? &stT : nullptr) :
                                               fill_triangle(hi, w2o, tv, tx, hu, hv, inside, (textured || hairOnMesh) ? &st : nullptr);
                if (hairOnMesh)
                    stT = st.tangent_u;
                if (textured)
                {
                    if constexpr (MTEX)
                    {
                        // base colour, roughness / metallic, Le: skh_material_probe's function
                        v3 Le = mk3(matLe.x, matLe.y, matLe.z);
                        resolve_material(sc.texels, sc.texDesc, sc.numTextures, mat, mte, Le, st.u, st.v);
                        matLe.x = Le.x, matLe.y = Le.y, matLe.z = Le.z; // (.w stays the material's luminance: the pdf is the table's)
                    }
                    else if (useBase)
                    {
                        const v4 c = tex_lookup_rgba8(sc.texels, sc.texDesc[mat.base_color_texture - 1u], st.u, st.v);
                        mat.base_color[0] = c.x, mat.base_color[1] = c.y, mat.base_color[2] = c.z;
                    }
                    if (useNormal)
                    {
                        const v4 c = tex_lookup_rgba8(sc.texels, sc.texDesc[mat.normal_texture - 1u], st.u, st.v);
                        const v3 ts = mk3(c.x * 2.0f - 1.0f, c.y * 2.0f - 1.0f, c.z * 2.0f - 1.0f);
                        sh.normal = normalize((st.tangent_u * ts.x + st.tangent_v * ts.y) + sh.normal * ts.z);
                    }
                }
                if (fp.debug == 1)
                    radiance = (sh.normal + mk3(1.0f)) * 0.5f, radianceDirty = true;
                else
                {
                    if constexpr (EMIT)
                    {
                        // an emissive mesh seen from its front side (the geometric normal before the `inside` flip): weighted as __closesthit__light weighs a
                        // light it hits, WITHOUT that branch's cosine (a Lambertian surface, as the sky); the path goes on below, the surface reflects too
                        if (hi.type == 0u && matLe.w > 0.0f)
                        {
                            const v3 ne = inside ? -sh.geom_normal : sh.geom_normal;
                            if (-dot(rayD, ne) > 0.0f)
                            {
                                const v3 Le = mk3(matLe.x, matLe.y, matLe.z);
                                SKH_RADIANCE_LOAD();
                                if (depth0 || specularBounce || !emit.nee)
                                    radiance = radiance + throughput * Le;
                                else
                                {
                                    const float lightPdf = emit_pdf(ne, matLe.w * emit.invSumW, sh.position, rayO) / (float)numPick;
                                    const float misWeight = mis_weight_balance(lastBsdfPdf, lightPdf);
                                    radiance = radiance + throughput * Le * misWeight;
                                }
                            }
                        }
                    }
                    const float xi0 = sampler_random_lut(smp, DIM_BSDF0, s_sobol), xi1 = sampler_random_lut(smp, DIM_BSDF1, s_sobol),
                                xi2 = sampler_random_lut(smp, DIM_BSDF2, s_sobol);
                    const float xi3 = HAIR ? sampler_random_lut(smp, DIM_BSDF3, s_sobol) : 0.0f; // (only the hair BSDF consumes xi.w)
                    const v3 k1 = -rayD;
                    BsdfSample bs;
                    SKH_SP(1) // hit reconstruction, material, textures, bsdf randoms
                    // estimateDirectLighting + sampleLight: closest_hit.cu:260-324 -- as a block of its own: a hit of a HAIR material (hair build) samples the light FIRST, so that
                    // the BSDF's two evaluations for this k1 -- the sampled direction's and the light sample's -- share the fibre geometry (hair_sample_and_evaluate); every
                    // other hit samples it where the reference does, behind the BSDF sample's event type.  The values do not depend on the order.
                    v3 toLight = mk3(0.0f);
                    float lightPdf = 0.0f;
                    v3 lrad = mk3(0.0f);
                    bool wantShadow = false;
                    float distToLight = 0.0f;
                    auto sampleLight = [&]() {
                        if (numPick > 0)
                        {
                            const float u = sampler_random_lut(smp, DIM_LIGHT_ID, s_sobol);
                            const uint32_t lightId = (uint32_t)((float)numPick * u);
                            const float lightSelectionPdf = 1.0f / (float)numPick;
                            if constexpr (EMIT)
                            {
                                if (emit.nee && lightId + 1u >= numPick)
                                {
                                    // the emitter set: the last entry of the pick.  The triangle from the fraction of the pick's own draw (no new dimension, its stratification survives)
                                    const float uSel = fminf(fmaxf((float)numPick * u - (float)(numPick - 1u), 0.0f), 0.99999994f);
                                    const float ux = sampler_random_lut(smp, DIM_LIGHT_X, s_sobol), uy = sampler_random_lut(smp, DIM_LIGHT_Y, s_sobol);
                                    const EmitSample es = emit_sample(emit, uSel, ux, uy, sh.position);
                                    toLight = es.L;
                                    if (dot(sh.normal, es.L) > 0.0f && -dot(es.L, es.normal) > 0.0f && es.pdf > 0.0f)
                                    {
                                        wantShadow = true;
                                        distToLight = es.dist * (1.0f - SKH_EMIT_SHADOW_MARGIN); // (ends short of the emitter itself: skh_device.h)
                                        lightPdf = es.pdf;
                                        lrad = es.Le; // (no second cosine, as for the environment: bsdf_evaluate carries the surface's)
                                        if constexpr (MTEX)
                                            lrad = lrad * emit_sample_texel(mtex, sc, es.instance, es.prim, ux, uy);
                                    }
                                    lightPdf *= lightSelectionPdf;
                                    return;
                                }
                            }
                            if constexpr (ENV)
                            {
                                if (lightId >= sc.numLights)
                                {
                                    // the environment: entry numLights of the pick.  No normal, no area; the shadow ray is a distant light's.
                                    const float ux = sampler_random_lut(smp, DIM_LIGHT_X, s_sobol), uy = sampler_random_lut(smp, DIM_LIGHT_Y, s_sobol);
                                    const EnvSample es = env_sample(env, ux, uy);
                                    toLight = es.dir;
                                    if (dot(sh.normal, es.dir) > 0.0f && es.ev.pdf > 0.0f)
                                    {
                                        wantShadow = true;
                                        distToLight = 1e9f;
                                        lightPdf = es.ev.pdf;
                                        // (no cosine here: bsdf_evaluate's value carries the surface's, as MDL's does.  The reference's light branch below multiplies by
                                        // a second one -- its lights are cosine emitters through it --; a sky is not, and the closed forms of tests/test_gpu_env.py hold the estimator to that)
                                        lrad = es.ev.Le;
                                    }
                                    lightPdf *= lightSelectionPdf;
                                    return;
                                }
                            }
                            // the whole 112-byte record in one round trip (by reference its fields were fetched in three dependent
                            // steps: type, then the branch's points, then colour / normal)
                            const Light light = sc.lights[lightId];
                            Lshape lse;
                            if constexpr (LSHAPE) // (the 32-byte shape entry in the same round trip: it hangs off the light's index only, not off the type test)
                                lse = lshape_fetch(lsh, lightId);
                            asm volatile("" ::"v"(light.points[0].x), "v"(light.points[1].x), "v"(light.points[2].x), "v"(light.points[3].x),
                                         "v"(light.color.x), "v"(light.normal.x), "v"(light.type));
                            if constexpr (LSHAPE)
                                asm volatile("" ::"v"(lse.flags), "v"(lse.axis.x));
                            const float ux = sampler_random_lut(smp, DIM_LIGHT_X, s_sobol), uy = sampler_random_lut(smp, DIM_LIGHT_Y, s_sobol);
                            LightSample d;
                            d.pointOnLight = mk3(0.0f);
                            d.pdf = 0.0f;
                            d.normal = mk3(0.0f);
                            d.area = 0.0f;
                            d.L = mk3(0.0f);
                            d.distToLight = 0.0f;
                            switch (light.type)
                            {
                            case 0:
                                d = fp.rectMethod == 0 ? sample_rect_light_uniform(light, ux, uy, sh.position) :
                                                         sample_rect_light(light, ux, uy, sh.position);
                                break;
                            case 1:
                                if constexpr (LSHAPE) // (a disk without the flag stays the zero sample it was)
                                {
                                    if (lse.flags & SKH_LSHAPE_SAMPLE_DISC)
                                        d = sample_disc_light(light, ux, uy, sh.position);
                                }
                                break;
                            case 2:
                                d = sample_sphere_light(light, ux, uy, sh.position);
                                break;
                            case 3:
                                d = sample_distant_light(light, ux, uy);
                                break;
                            default:
                                break;
                            }
                            toLight = d.L;
                            v3 Li = mk3(light.color);
                            if constexpr (LSHAPE) // (s = 0: Li = 0 fails all3 below -- a dark direction queues no shadow ray; pdf and pick stay what they are)
                                Li = Li * lshape_cone(lse, -d.L);
                            if (dot(sh.normal, d.L) > 0.0f && -dot(d.L, d.normal) > 0.0f && all3(Li))
                            {
                                wantShadow = true;
                                distToLight = d.distToLight;
                                lightPdf = d.pdf;
                                lrad = 1.0f * Li * saturatef(dot(sh.normal, d.L)); // visibility applied by k_trace<shadow>
                            }
                            lightPdf *= lightSelectionPdf;
                        }
                    };
                    const bool hairHit = HAIR && mat.type == 3u;
                    BsdfEval evHair;
                    bool evHairDone = false;
                    if (hairHit)
                    {
                        sampleLight();
                        // (the evaluation is wanted exactly where the flow below would ask for it, should the sampled event not be an absorption)
                        evHairDone = !(isnan3(lrad) || isnan(lightPdf)) && (((dot(toLight, sh.normal) > 0.0f) != inside) && lightPdf != 0.0f);
                        hair_sample_and_evaluate(mat, sh.normal, sh.geom_normal, stT, k1, xi0, xi1, xi2, xi3, sc.hairConst + (mid < sc.numMaterials ? mid : 0u), bs, evHairDone, toLight, evHair);
                    }
                    else
                        bsdf_sample<HAIR>(mat, sh.normal, sh.geom_normal, stT, k1, xi0, xi1, xi2, xi3, inside, bs, HAIR ? sc.hairConst + (mid < sc.numMaterials ? mid : 0u) : nullptr);
                    SKH_SP(2) // bsdf_sample
                    if (bs.event_type == EV_ABSORB)
                    {
                        if (depth0)
                            firstEvent = 1; // eAbsorb
                        throughput = mk3(0.0f);
                    }
                    else
                    {
                        specularBounce = (bs.event_type & EV_SPECULAR) != 0;
                        if (depth0)
                        {
                            if (bs.event_type & EV_DIFFUSE)
                                firstEvent = 2;
                            if (bs.event_type & EV_GLOSSY)
                                firstEvent = 3;
                        }
                        bool errorOut = false;
                        if (bs.event_type & (EV_DIFFUSE | EV_GLOSSY))
                        {
                            if (!hairHit)
                                sampleLight();
                            if (isnan3(lrad) || isnan(lightPdf))
                            {
                                radiance = mk3(10000.0f, 0.0f, 0.0f), radianceDirty = true;
                                throughput = mk3(0.0f);
                                errorOut = true;
                            }
                            else
                            {
                                const bool isNextEventValid = ((dot(toLight, sh.normal) > 0.0f) != inside) && lightPdf != 0.0f;
                                if (isNextEventValid)
                                {
                                    BsdfEval ev;
                                    SKH_SP(3) // light sampling
                                    if (hairHit)
                                        ev = evHair; // (evaluated beside the sample: evHairDone holds exactly when this branch is reached)
                                    else
                                        bsdf_evaluate<HAIR>(mat, sh.normal, sh.geom_normal, stT, k1, toLight, inside, ev, HAIR ? sc.hairConst + (mid < sc.numMaterials ? mid : 0u) : nullptr);
                                    SKH_SP(4) // bsdf_evaluate
                                    if (isnan3(ev.bsdf_diffuse) || isnan3(ev.bsdf_glossy))
                                    {
                                        radiance = mk3(10000.0f, 0.0f, 0.0f), radianceDirty = true;
                                        throughput = mk3(0.0f);
                                        errorOut = true;
                                    }
                                    else if (ev.pdf > 0.0f && wantShadow)
                                    {
                                        const v3 radianceOverPdf = lrad / lightPdf;
                                        const float misWeight = mis_weight_balance(lightPdf, ev.pdf);
                                        shC = throughput * radianceOverPdf * misWeight * (ev.bsdf_diffuse + ev.bsdf_glossy);
                                        shO = offset_ray(sh.position, sh.geom_normal);
                                        shD = toLight;
                                        shTmax = distToLight;
                                        emitShadow = true;
                                    }
                                }
                            }
                        }
                        if (!kLast && !errorOut) // (the last bounce has no continuation: nothing below outlives it)
                        {
                            if (bs.event_type & EV_TRANSMISSION)
                            {
                                inside = !inside;
                                origin = offset_ray(sh.position, -sh.geom_normal);
                            }
                            else
                                origin = offset_ray(sh.position, sh.geom_normal);
                            lastBsdfPdf = specularBounce ? 1.0f : bs.pdf;
                            dir = bs.k2;
                            throughput = throughput * bs.bsdf_over_pdf;
                        }
                    }
                }
            }
        }
        SKH_SP(5) // rest of the hit program
        if constexpr (kLast)
        {
            // depth + 1 == maxDepth: the tail of the bounce loop (OptixRender.cu:131-153) ends every path here whatever the roulette says, and nothing
            // reads the throughput, lastBsdfPdf or the flags again (the event bits are bounce 0's): only the radiance record is written
            if (radianceDirty)
                ps.rad()[pid] = make_float4(radiance.x, radiance.y, radiance.z, 0.0f);
        }
        else
        {
            // tail of the bounce loop: OptixRender.cu:131-153
            bool alive = true;
            if (prdDepth > 3)
            {
                const float p = fmaxf(throughput.x, fmaxf(throughput.y, throughput.z));
                if (sampler_random_lut(smp, DIM_RR, s_sobol) > p)
                    alive = false;
                else
                    throughput = throughput * (1.0f / (p + 1e-5f));
            }
            if (alive && dot(throughput, throughput) < 1e-5f)
                alive = false;
            if (alive)
            {
                ++prdDepth;
                if (fp.debug == 1)
                    alive = false;
            }
            if (alive && prdDepth >= fp.maxDepth)
                alive = false;
            emitNext = alive;
            nextO = origin;
            nextD = dir;
            // write back path state
            P[pid] = throughput.x;
            P[pid + S] = throughput.y;
            P[pid + 2 * S] = throughput.z;
            if (radianceDirty)
            {
                ps.rad()[pid] = make_float4(radiance.x, radiance.y, radiance.z, 0.0f);
            }
            P[pid + 6 * S] = lastBsdfPdf;
            reinterpret_cast<uint32_t*>(P)[pid + 7 * S] =
                (inside ? PF_INSIDE : 0u) | (specularBounce ? PF_SPECULAR : 0u) | (firstEvent << PF_EVENT_SHIFT);
        }
#undef SKH_RADIANCE_LOAD
    }
    SKH_SP(6) // bounce tail + path-state write
    // stream compaction of live paths / shadow rays: one atomic per queue per workgroup, both in flight together
    uint32_t ni = 0, si;
    if constexpr (kLast) // (the shadow queue alone: no ballot, prefix, atomic or store for a next queue that stays empty)
        si = block_compact(emitShadow, shadowCount + shard * SKH_COUNT_STRIDE, s_wave, false);
    else
        block_compact2(emitNext, nextCount + shard * SKH_COUNT_STRIDE, emitShadow, shadowCount + shard * SKH_COUNT_STRIDE, s_wave, ni, si);
    ni += shard * nextQ.region; // (a shard's output never outgrows its region: at most one ray of either kind per input ray)
    si += shard * shadowQ.region;
    if (!kLast && emitNext)
    {
        nextQ.plane(0)[ni] = nextO.x;
        nextQ.plane(1)[ni] = nextO.y;
        nextQ.plane(2)[ni] = nextO.z;
        nextQ.plane(3)[ni] = nextD.x;
        nextQ.plane(4)[ni] = nextD.y;
        nextQ.plane(5)[ni] = nextD.z;
        // (planes 6 / 7, tmin / tmax: constants of the pass, filled once by the host -- k_fill_f32 in render_one)
        nextQ.ids()[ni] = pid;
    }
    if (emitShadow)
    {
        shadowQ.plane(0)[si] = shO.x;
        shadowQ.plane(1)[si] = shO.y;
        shadowQ.plane(2)[si] = shO.z;
        shadowQ.plane(3)[si] = shD.x;
        shadowQ.plane(4)[si] = shD.y;
        shadowQ.plane(5)[si] = shD.z;
        // (plane 6 = shadowTmin: filled once by the host)
        shadowQ.plane(7)[si] = shTmax;
        // (the path id travels with the contribution -- one 16-byte record the any-hit launch reads back with ONE scattered load -- not in the queue's id plane)
        contrib[si] = make_float4(shC.x, shC.y, shC.z, __uint_as_float(pid));
    }
#ifdef SKH_LANE_PROFILE
    SKH_SP(7) // compaction + queue writes
    for (int k = 0; k < 8; ++k)
    {
        const uint32_t hi32 = wave_max((uint32_t)(spc[k] >> 4));
        if ((threadIdx.x & 63u) == 0)
            atomicAdd(&sc.profile->shade[k], (unsigned long long)hi32 << 4);
    }
#endif
#undef SKH_SP
