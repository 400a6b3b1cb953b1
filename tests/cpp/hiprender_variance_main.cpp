// oka::HipRender::setVarianceGuidance (the mirror build: strelka_amd/host/liboka_hip.so) behind hdRunner's frame loop:
//   hiprender_variance <outdir> <scene.skscene>
// The sequence still, still, move, move, still of hiprender_temporal_main.cpp (a move shifts the camera by 0.1 in x), every frame's output image (tonemapped, as
// map() hands it back) written out, by four renderers on the same scene, all with temporal accumulation (every default) and the denoiser (sigmaColor 0.2, four
// levels) on:
//   tpdn_<f>.bin    one that never heard of variance guidance
//   off_<f>.bin     one whose variance guidance was turned on and off again before the first frame
//   vg_<f>.bin      one with it on (every default)
// and one with temporal accumulation and variance guidance but WITHOUT the denoiser (no image written: the setting must not act).
// Per frame of the third, for the ctypes path to make the same calls: vg_aov_<f>.bin, vg_temporal_<f>.bin, vg_variance_<f>.bin (the skh_vdenoise_params of the
// last guided call) and a line of vg_calls.txt:
//   subframe_index enable_accumulation hadPrevious hadPreviousMoments  temporal moments vdenoise denoise     (the last four: calls made during this frame)
// Once: the scene arrays as the adapter uploaded them and denoise_params.bin.
// counts.txt: skh_moments and skh_denoise_variance calls of the first, second and fourth renderer (six zeros); then, of the third after a resize to 64 x 48:
// hadPreviousMoments of a moving frame right after the resize (0: the moments were dropped) and of the next moving frame (1).
#include "../../strelka_amd/host/oka_render.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace oka;

template <typename T>
static bool dump(const std::string& dir, const std::string& name, const T* data, size_t n)
{
    FILE* f = fopen((dir + "/" + name).c_str(), "wb");
    if (!f)
        return false;
    const bool ok = fwrite(data, sizeof(T), n, f) == n;
    return fclose(f) == 0 && ok;
}

static const uint32_t W = 96, H = 64;
static const int FRAMES = 5;
static const bool MOVES[FRAMES] = { false, false, true, true, false };

struct Calls
{
    unsigned long long temporal = 0, moments = 0, vdenoise = 0, denoise = 0;
};

struct Session
{
    SettingsManager sm;
    SharedContext ctx;
    Scene scene;
    Render* render = nullptr;
    HipRender* hr = nullptr;
    Buffer* out = nullptr;
    bool open(const char* path, bool denoiser)
    {
        if (!scene.loadDump(path))
            return false;
        ctx.mSettingsManager = &sm;
        sm.setAs<uint32_t>("render/width", W);
        sm.setAs<uint32_t>("render/height", H);
        sm.setAs<uint32_t>("render/pt/depth", 4);
        sm.setAs<uint32_t>("render/pt/sppTotal", 64);
        sm.setAs<uint32_t>("render/pt/spp", 1);
        sm.setAs<uint32_t>("render/pt/tonemapperType", 1);
        sm.setAs<uint32_t>("render/pt/debug", 0);
        sm.setAs<bool>("render/pt/enableAcc", true);
        sm.setAs<bool>("render/pt/isResized", false);
        sm.setAs<uint32_t>("render/pt/rectLightSamplingMethod", 0);
        sm.setAs<float>("render/post/tonemapper/filmIso", 100.0f);
        sm.setAs<float>("render/post/tonemapper/cm2_factor", 1.0f);
        sm.setAs<float>("render/post/tonemapper/fStop", 4.0f);
        sm.setAs<float>("render/post/tonemapper/shutterSpeed", 100.0f);
        sm.setAs<float>("render/post/gamma", 2.4f);
        sm.setAs<float>("render/pt/dev/shadowRayTmin", 0.0f);
        sm.setAs<float>("render/pt/dev/materialRayTmin", 0.0f);
        render = RenderFactory::createRender(RenderType::eCompute);
        render->setSharedContext(&ctx);
        ctx.mRender = render;
        render->setScene(&scene);
        render->init();
        hr = static_cast<HipRender*>(render);
        out = render->createBuffer(BufferDesc{ W, H, BufferFormat::FLOAT4 });
        HipDenoise dn;
        dn.levels = 4, dn.sigmaColor = 0.2f;
        return hr->setTemporal(true) && (!denoiser || hr->setDenoiser(true, &dn));
    }
    void move()
    {
        Camera& cam = scene.getCamera(0);
        cam.setPosition(float3{ cam.position.x + 0.1f, cam.position.y, cam.position.z });
    }
    Calls calls()
    {
        skh_temporal_info t = {};
        skh_moments_info m = {};
        skh_vdenoise_info v = {};
        skh_denoise_info d = {};
        skh_get_temporal_info(hr->context(), &t), skh_get_moments_info(hr->context(), &m), skh_get_vdenoise_info(hr->context(), &v), skh_get_denoise_info(hr->context(), &d);
        Calls c;
        c.temporal = t.calls, c.moments = m.calls, c.vdenoise = v.calls, c.denoise = d.calls;
        return c;
    }
    bool sequence(const std::string& dir, const std::string& prefix, bool record)
    {
        FILE* log = record ? fopen((dir + "/" + prefix + "_calls.txt").c_str(), "w") : nullptr;
        if (record && !log)
            return false;
        bool ok = true;
        for (int f = 0; f < FRAMES && ok; ++f)
        {
            if (MOVES[f])
                move();
            const Calls before = calls();
            render->render(out);
            const Calls after = calls();
            out->map();
            ok = !prefix.empty() ? dump(dir, prefix + "_" + std::to_string(f) + ".bin", static_cast<const char*>(out->getHostPointer()), (size_t)W * H * 16) : true;
            if (!record || !ok)
                continue;
            skh_aov_params ap;
            skh_temporal_params tp;
            skh_vdenoise_params vp;
            bool had = false, hadMoments = false;
            uint32_t index = 0, accumulate = 0;
            if (!hr->aovParams(ap, nullptr, false) || !hr->temporalParams(tp, &had) || !hr->varianceParams(vp, &hadMoments))
                return false;
            hr->lastSample(index, accumulate);
            fprintf(log, "%u %u %d %d %llu %llu %llu %llu\n", index, accumulate, had ? 1 : 0, hadMoments ? 1 : 0, after.temporal - before.temporal,
                    after.moments - before.moments, after.vdenoise - before.vdenoise, after.denoise - before.denoise);
            ok = dump(dir, prefix + "_aov_" + std::to_string(f) + ".bin", &ap, 1) && dump(dir, prefix + "_temporal_" + std::to_string(f) + ".bin", &tp, 1) &&
                 dump(dir, prefix + "_variance_" + std::to_string(f) + ".bin", &vp, 1);
        }
        if (log)
            fclose(log);
        return ok;
    }
    ~Session()
    {
        delete out;
        delete render;
    }
};

int main(int argc, char** argv)
{
    if (argc < 3)
    {
        fprintf(stderr, "usage: hiprender_variance <outdir> <scene.skscene>\n");
        return 2;
    }
    const std::string dir = argv[1];
    unsigned long long counts[8] = {};
    {
        Session plain;
        if (!plain.open(argv[2], true))
            return 3;
        if (!plain.sequence(dir, "tpdn", false))
            return 4;
        counts[0] = plain.calls().moments, counts[1] = plain.calls().vdenoise;
        skh_denoise_params dp;
        if (!plain.hr->denoiseParams(dp) || !dump(dir, "denoise_params.bin", &dp, 1))
            return 8;
    }
    {
        Session off;
        if (!off.open(argv[2], true))
            return 3;
        if (!off.hr->setVarianceGuidance(true) || !off.hr->setVarianceGuidance(false))
            return 5;
        if (!off.sequence(dir, "off", false))
            return 4;
        counts[2] = off.calls().moments, counts[3] = off.calls().vdenoise;
    }
    {
        Session alone; // without the denoiser the setting does not act
        if (!alone.open(argv[2], false))
            return 3;
        if (!alone.hr->setVarianceGuidance(true))
            return 5;
        if (!alone.sequence(dir, "", false))
            return 4;
        counts[4] = alone.calls().moments, counts[5] = alone.calls().vdenoise;
    }
    Session vg;
    if (!vg.open(argv[2], true))
        return 3;
    // a setting the library refuses is refused here, and the previous one stays
    HipVariance bad;
    bad.minHistory = 0.5f;
    if (vg.hr->setVarianceGuidance(true, &bad) || vg.hr->lastError().empty())
        return 7;
    if (!vg.hr->setVarianceGuidance(true))
        return 5;
    Scene& scene = vg.scene;
    std::vector<skh_instance> inst(scene.getInstances().size());
    for (size_t i = 0; i < inst.size(); ++i)
    {
        const Instance& in = scene.getInstances()[i];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c)
                inst[i].transform[4 * r + c] = in.transform.m[c][r];
        inst[i].type = (uint32_t)in.type, inst[i].geom_id = in.mMeshId, inst[i].material_id = in.mMaterialId, inst[i].light_id = in.mLightId;
    }
    std::vector<skh_material> mats;
    for (auto& m : scene.getMaterials())
        mats.push_back(m.args);
    if (!vg.sequence(dir, "vg", true))
        return 4;
    skh_aov_params ap;
    if (!vg.hr->aovParams(ap, nullptr, false))
        return 8;
    float mtx[32];
    memcpy(mtx, ap.view_to_world, 64), memcpy(mtx + 16, ap.clip_to_view, 64);
    if (!dump(dir, "vertices.bin", scene.getVertices().data(), scene.getVertices().size()) || !dump(dir, "indices.bin", scene.getIndices().data(), scene.getIndices().size()) ||
        !dump(dir, "meshes.bin", scene.getMeshes().data(), scene.getMeshes().size()) || !dump(dir, "lights.bin", scene.getLights().data(), scene.getLights().size()) ||
        !dump(dir, "instances.bin", inst.data(), inst.size()) || !dump(dir, "materials.bin", mats.data(), mats.size()) || !dump(dir, "camera.bin", mtx, 32))
        return 4;
    // a resize drops the moments with the history: the first moving frame after it has no previous moments, the next one has
    Buffer* small = vg.render->createBuffer(BufferDesc{ 64, 48, BufferFormat::FLOAT4 });
    skh_vdenoise_params vp;
    bool hadMoments = true;
    vg.move();
    vg.render->render(small);
    if (!vg.hr->varianceParams(vp, &hadMoments) || vp.width != 64u || vp.height != 48u)
        return 9;
    counts[6] = hadMoments ? 1 : 0;
    vg.move();
    vg.render->render(small);
    if (!vg.hr->varianceParams(vp, &hadMoments))
        return 9;
    counts[7] = hadMoments ? 1 : 0;
    delete small;
    FILE* ft = fopen((dir + "/counts.txt").c_str(), "w");
    if (!ft)
        return 4;
    for (unsigned long long c : counts)
        fprintf(ft, "%llu ", c);
    fprintf(ft, "\n");
    fclose(ft);
    printf("hiprender_variance ok\n");
    return 0;
}
