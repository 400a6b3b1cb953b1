// skh_probes.inc -- host side and kernels of the probes that stand apart from the renderer (part of strelka_hip.hip's translation unit): skh_probe_memory, and the
// tests' doors to the BSDFs (skh_bsdf_probe) and to single device functions (skh_unit_probe).  The probes of the features stay beside their features.

// ---- memory ceilings of this GPU, measured with the access shapes of the hot path (include/strelka_hip.h: skh_probe_memory) ----
__global__ __launch_bounds__(256) void k_probe_fill(uint4* __restrict__ buf, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    {
        const uint32_t h = hash_murmur((uint32_t)i * 0x9e3779b9u + (uint32_t)(i >> 32));
        buf[i] = make_uint4(h, h * 0x85ebca6bu, h ^ 0xc2b2ae35u, h * 0x27d4eb2fu + 1u);
    }
}

__global__ __launch_bounds__(256) void k_probe_copy(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

// one-wave workgroups like k_trace; every lane fetches `perLane` records of R uint4 (R = 4: 64 bytes = one BVH node) at pseudo-random,
// record-aligned places of the buffer.  DEPENDENT: the next place comes out of the record just loaded (a traversal step); otherwise
// four fetches are in flight.
template <bool DEPENDENT, int R>
__global__ __launch_bounds__(SKH_TRACE_BLOCK) void k_probe_gather(const uint4* __restrict__ buf, uint32_t nRec, uint32_t perLane, uint32_t* __restrict__ sink)
{
    uint32_t s = hash_murmur(blockIdx.x * SKH_TRACE_BLOCK + threadIdx.x + 1u);
    uint32_t acc = 0u;
    if (DEPENDENT)
    {
        for (uint32_t i = 0; i < perLane; ++i)
        {
            const uint4* p = buf + R * (size_t)__umulhi(s, nRec);
            uint32_t x = 0u;
#pragma unroll
            for (int j = 0; j < R; ++j)
            {
                const uint4 a = p[j];
                x ^= a.x ^ a.y ^ a.z ^ a.w;
            }
            acc += x;
            s = s * 1664525u + 1013904223u + x;
        }
    }
    else
    {
        for (uint32_t i = 0; i < perLane; i += 4)
        {
            uint4 v[4][R];
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                const uint4* p = buf + R * (size_t)__umulhi(s, nRec);
                s = s * 1664525u + 1013904223u;
#pragma unroll
                for (int j = 0; j < R; ++j)
                    v[k][j] = p[j];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < R; ++j)
                    acc += v[k][j].x ^ v[k][j].y ^ v[k][j].z ^ v[k][j].w;
        }
    }
    if (acc == 0x12345u) // (keeps the loads alive; practically never true)
        sink[0] = s;
}

skh_status skh_probe_memory(skh_context* c, uint32_t kind, uint64_t bytes, uint32_t record_bytes, uint32_t repeat, double* out_gbps, double* out_ms)
{
    if (!c || kind > SKH_PROBE_CHASE || bytes < (1u << 20) || !out_gbps ||
        (kind != SKH_PROBE_COPY && record_bytes != 32 && record_bytes != 64 && record_bytes != 128))
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    DevBuf a, b;
    const size_t n16 = (size_t)(bytes / 64) * 4; // uint4 elements, whole 64-byte records
    SKH_CHECK(dev_alloc(c, a, n16 * 16));
    if (kind == SKH_PROBE_COPY)
        SKH_CHECK(dev_alloc(c, b, n16 * 16));
    struct Events // (destroyed on every exit)
    {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events()
        {
            if (e0)
                (void)hipEventDestroy(e0);
            if (e1)
                (void)hipEventDestroy(e1);
        }
    } ev;
    hipEvent_t &e0 = ev.e0, &e1 = ev.e1;
    const uint32_t grid = (uint32_t)c->dev.numCUs * c->opt.wavesPerCU; // the trace kernels' grid
    const uint32_t perLane = 256;
    repeat = std::max(1u, repeat);
    k_probe_fill<<<c->dev.numCUs * 8, 256, 0, c->dev.stream>>>(a.as<uint4>(), n16);
    double moved = 0.0;
    for (uint32_t r = 0; r <= repeat; ++r) // (pass 0 is the warm-up)
    {
        if (r == 1)
        {
            if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, c->dev.stream) != hipSuccess)
            {
                c->dev.err = "skh_probe_memory: hipEvent";
                return SKH_FAIL;
            }
        }
        if (kind == SKH_PROBE_COPY)
        {
            k_probe_copy<<<c->dev.numCUs * 16, 256, 0, c->dev.stream>>>(a.as<uint4>(), b.as<uint4>(), n16);
            moved = 2.0 * 16.0 * (double)n16;
        }
        else
        {
            const uint32_t nRec = (uint32_t)(n16 * 16 / record_bytes);
            uint32_t* sink = a.as<uint32_t>();
            // (the build by dependence and uint4s per record)
            static const decltype(&k_probe_gather<false, 2>) kGather[2][3] = { { k_probe_gather<false, 2>, k_probe_gather<false, 4>, k_probe_gather<false, 8> },
                                                                                { k_probe_gather<true, 2>, k_probe_gather<true, 4>, k_probe_gather<true, 8> } };
            kGather[kind == SKH_PROBE_CHASE ? 1 : 0][record_bytes == 32 ? 0 : record_bytes == 64 ? 1 : 2]<<<grid, SKH_TRACE_BLOCK, 0, c->dev.stream>>>(a.as<uint4>(), nRec, perLane, sink);
            moved = (double)record_bytes * perLane * SKH_TRACE_BLOCK * (double)grid;
        }
    }
    float ms = 0.0f;
    if (hipEventRecord(e1, c->dev.stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
    {
        c->dev.err = "skh_probe_memory: timing failed";
        return SKH_FAIL;
    }
    ms /= (float)repeat;
    *out_gbps = moved / (ms * 1e-3) / 1e9;
    if (out_ms)
        *out_ms = ms;
    return SKH_OK;
}

// ---- BSDF probes (tests) ----
static_assert(sizeof(skh_bsdf_query) == 84 && sizeof(skh_bsdf_result) == 64, "ABI layout");
__global__ void k_bsdf_probe(const skh_bsdf_query* __restrict__ q, uint32_t n, const Material* __restrict__ mats, uint32_t numMaterials,
                             skh_bsdf_result* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const skh_bsdf_query in = q[i];
    const Material m = mats[in.material < numMaterials ? in.material : 0u];
    const v3 N = mk3(in.normal[0], in.normal[1], in.normal[2]), Ng = mk3(in.geom_normal[0], in.geom_normal[1], in.geom_normal[2]);
    const v3 T = mk3(in.tangent_u[0], in.tangent_u[1], in.tangent_u[2]);
    const v3 k1 = mk3(in.k1[0], in.k1[1], in.k1[2]), k2 = mk3(in.k2[0], in.k2[1], in.k2[2]);
    const HairConst hc = hair_const(m); // (what k_hair_consts tabulates per material for k_shade)
    BsdfSample bs;
    bsdf_sample<true>(m, N, Ng, T, k1, in.xi[0], in.xi[1], in.xi[2], in.xi[3], in.inside != 0u, bs, &hc);
    BsdfEval ev;
    bsdf_evaluate<true>(m, N, Ng, T, k1, k2, in.inside != 0u, ev, &hc);
    skh_bsdf_result r;
    r.k2[0] = bs.k2.x, r.k2[1] = bs.k2.y, r.k2[2] = bs.k2.z;
    r.bsdf_over_pdf[0] = bs.bsdf_over_pdf.x, r.bsdf_over_pdf[1] = bs.bsdf_over_pdf.y, r.bsdf_over_pdf[2] = bs.bsdf_over_pdf.z;
    r.pdf = bs.pdf;
    r.event_type = bs.event_type;
    r.bsdf_diffuse[0] = ev.bsdf_diffuse.x, r.bsdf_diffuse[1] = ev.bsdf_diffuse.y, r.bsdf_diffuse[2] = ev.bsdf_diffuse.z;
    r.bsdf_glossy[0] = ev.bsdf_glossy.x, r.bsdf_glossy[1] = ev.bsdf_glossy.y, r.bsdf_glossy[2] = ev.bsdf_glossy.z;
    r.eval_pdf = ev.pdf;
    r.reserved0 = 0u;
    out[i] = r;
}

skh_status skh_bsdf_probe(skh_context* c, const skh_bsdf_query* queries, uint32_t n, skh_bsdf_result* results)
{
    if (!c || (n && (!queries || !results)))
        return SKH_INVALID_ARGUMENT;
    (void)hipSetDevice(c->dev.device);
    if (n == 0)
        return SKH_OK;
    if (c->scene.nMaterials == 0)
    {
        c->dev.err = "skh_bsdf_probe: call skh_set_materials first";
        return SKH_INVALID_ARGUMENT;
    }
    const ProbeIn in[] = { { queries, sizeof(skh_bsdf_query) * (size_t)n } };
    return probe_roundtrip(c, in, results, sizeof(skh_bsdf_result) * (size_t)n, [&](const DevBuf* d, const DevBuf& dOut) {
        k_bsdf_probe<<<(n + 127) / 128, 128, 0, c->dev.stream>>>(d[0].as<skh_bsdf_query>(), n, c->scene.dMaterials.as<Material>(), c->scene.nMaterials, dOut.as<skh_bsdf_result>());
    });
}

// ---- unit probes (tests): the device functions of the sampler, the light samplers and the accumulator, one call per record, so that
// GPU tests can hold the HIP code against the reference-generated fixtures of tests/golden/ directly ----
static const uint32_t kUnitIn[SKH_UNIT_COUNT] = { 20, 8, 20, 24, 12, 8, 12, 12, 8, 8, 12 }, kUnitOut[SKH_UNIT_COUNT] = { 12, 4, 48, 4, 16, 4, 12, 24, 40, 36, 24 };
static const uint32_t kUnitConst[SKH_UNIT_COUNT] = { 0, 0, 112, 112, 112, 0, 12, 12, 0, 0, 0 };
__global__ void __launch_bounds__(256) k_unit_probe(uint32_t unit, uint32_t param, const float* __restrict__ consts, const uint32_t* __restrict__ in, uint32_t n,
                                                    uint32_t* __restrict__ out)
{
    __shared__ uint32_t s_lut[SKH_SOBOL_LUT_WORDS]; // the byte-folded Sobol table as k_shade stages it
    for (uint32_t k = threadIdx.x; k < SKH_SOBOL_LUT_WORDS; k += blockDim.x)
        s_lut[k] = g_sobol_lut[k];
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float* fin = reinterpret_cast<const float*>(in);
    float* fout = reinterpret_cast<float*>(out);
    Light l;
    if (unit == SKH_UNIT_LIGHT_SAMPLE || unit == SKH_UNIT_LIGHT_PDF || unit == SKH_UNIT_LIGHT_NORMAL)
        l = *reinterpret_cast<const Light*>(consts);
    switch (unit)
    {
    case SKH_UNIT_SAMPLER: {
        const uint32_t* r = in + 5 * (size_t)i;
        Sampler s = init_sampler(r[0], r[1], r[2], param, 52u); // seed 52: OptixRender.cu:101
        s.depth = r[3];
        out[3 * (size_t)i] = __float_as_uint(sampler_random(s, r[4]));
        out[3 * (size_t)i + 1] = __float_as_uint(sampler_random_lut(s, r[4], s_lut));
        out[3 * (size_t)i + 2] = s.sampleIdx;
        break;
    }
    case SKH_UNIT_SOBOL:
        out[i] = sobol_uint(in[2 * (size_t)i], in[2 * (size_t)i + 1]);
        break;
    case SKH_UNIT_LIGHT_SAMPLE: {
        const float* r = fin + 5 * (size_t)i;
        const v3 P = mk3(r[0], r[1], r[2]);
        LightSample d;
        if (param == 0)
            d = sample_rect_light_uniform(l, r[3], r[4], P);
        else if (param == 1)
            d = sample_rect_light(l, r[3], r[4], P);
        else if (param == 2)
            d = sample_sphere_light(l, r[3], r[4], P);
        else
            d = sample_distant_light(l, r[3], r[4]);
        float* o = fout + 12 * (size_t)i;
        o[0] = d.pointOnLight.x, o[1] = d.pointOnLight.y, o[2] = d.pointOnLight.z, o[3] = d.pdf;
        o[4] = d.normal.x, o[5] = d.normal.y, o[6] = d.normal.z, o[7] = d.area;
        o[8] = d.L.x, o[9] = d.L.y, o[10] = d.L.z, o[11] = d.distToLight;
        break;
    }
    case SKH_UNIT_LIGHT_PDF: {
        const float* r = fin + 6 * (size_t)i;
        fout[i] = get_light_pdf(l, mk3(r[0], r[1], r[2]), mk3(r[3], r[4], r[5]));
        break;
    }
    case SKH_UNIT_LIGHT_NORMAL: {
        const float* r = fin + 3 * (size_t)i;
        const v3 nn = calc_light_normal(l, mk3(r[0], r[1], r[2]));
        fout[4 * (size_t)i] = nn.x, fout[4 * (size_t)i + 1] = nn.y, fout[4 * (size_t)i + 2] = nn.z, fout[4 * (size_t)i + 3] = calc_light_area(l);
        break;
    }
    case SKH_UNIT_MIS:
        fout[i] = mis_weight_balance(fin[2 * (size_t)i], fin[2 * (size_t)i + 1]);
        break;
    case SKH_UNIT_ACCUMULATE: {
        // a SEQUENCE: record k is folded into the running value of records 0..k-1 (sub-frame index param + k): one thread
        if (i != 0)
            return;
        const v3 e = mk3(consts[0], consts[1], consts[2]);
        v3 prev = mk3(0.0f);
        for (uint32_t k = 0; k < n; ++k)
        {
            prev = accumulate(prev, mk3(fin[3 * (size_t)k], fin[3 * (size_t)k + 1], fin[3 * (size_t)k + 2]), e, param + k);
            fout[3 * (size_t)k] = prev.x, fout[3 * (size_t)k + 1] = prev.y, fout[3 * (size_t)k + 2] = prev.z;
        }
        break;
    }
    case SKH_UNIT_TONEMAP: {
        const v3 e = mk3(consts[0], consts[1], consts[2]);
        const v3 c = mk3(fin[3 * (size_t)i], fin[3 * (size_t)i + 1], fin[3 * (size_t)i + 2]);
        const v3 t = tonemap(c, e), iv = inverse_tonemap(c, e);
        float* o = fout + 6 * (size_t)i;
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = iv.x, o[4] = iv.y, o[5] = iv.z;
        break;
    }
    case SKH_UNIT_LIBM: {
        // skh_libm.h on the device: the bits the CPU checker's copy of the same text must reproduce
        const float x = fin[2 * (size_t)i], y = fin[2 * (size_t)i + 1];
        float* o = fout + 10 * (size_t)i;
        o[0] = skm::sinf_(x), o[1] = skm::cosf_(x), o[2] = skm::acosf_(x), o[3] = skm::asinf_(x), o[4] = skm::atan2f_(y, x);
        o[5] = skm::expf_(x), o[6] = skm::logf_(x), o[7] = skm::sinhf_(x), o[8] = skm::powf_(x, y), o[9] = skm::atan2f_(x, y);
        break;
    }
    default:
        break;
    }
}

skh_status skh_unit_probe(skh_context* c, uint32_t unit, uint32_t param, const void* consts, const void* in, uint32_t n, void* out)
{
    if (!c || unit >= SKH_UNIT_COUNT || (n && (!in || !out)) || (kUnitConst[unit] && !consts))
    {
        if (c)
            c->dev.err = "skh_unit_probe: unknown unit, or a missing input / output / constants pointer";
        return SKH_INVALID_ARGUMENT;
    }
    const bool envUnit = unit == SKH_UNIT_ENV_SAMPLE || unit == SKH_UNIT_ENV_EVAL;
    if (envUnit && c->env.w == 0)
    {
        c->dev.err = "skh_unit_probe: the context has no environment";
        return SKH_INVALID_ARGUMENT;
    }
    (void)hipSetDevice(c->dev.device);
    if (n == 0)
        return SKH_OK;
    const ProbeIn pin[] = { { in, (size_t)kUnitIn[unit] * n }, { consts, kUnitConst[unit] } }; // (the Sobol tables were uploaded by skh_create)
    return probe_roundtrip(c, pin, out, (size_t)kUnitOut[unit] * n, [&](const DevBuf* d, const DevBuf& dOut) {
        if (envUnit)
            k_env_probe<<<(n + 255) / 256, 256, 0, c->dev.stream>>>(make_env(c), unit == SKH_UNIT_ENV_SAMPLE ? 1u : 0u, d[0].as<float>(), n, dOut.as<uint32_t>());
        else
            k_unit_probe<<<(n + 255) / 256, 256, 0, c->dev.stream>>>(unit, param, d[1].as<float>(), d[0].as<uint32_t>(), n, dOut.as<uint32_t>());
    });
}
