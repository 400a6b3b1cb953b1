// oka::HipRender::setHistoryRectification (the mirror build: strelka_amd/host/liboka_hip.so) behind hdRunner's frame loop:
//   hiprender_rectify_render <outdir> <scene.skscene>
// The sequence still, move-instance, move-instance, still (four frames; a move carries instance 1, the panel, by 0.1 in x and 0.05 in y through
// Scene::updateInstanceTransform), the camera at rest, every frame's output image (tonemapped, as map() hands it back) written out, by renderers on the same
// scene, all with temporal accumulation and object motion on:
//   plain_<f>.bin   a HipRender that never heard of history rectification
//   off_<f>.bin     one whose history rectification was turned on and off again before the first frame
//   on_<f>.bin      one with it on, every default
//   ondn_<f>.bin    one with it on, the denoiser (sigmaColor 0.2, four levels) and variance guidance on: the guided path
// <p>_calls.txt, a line per frame: hadPrevious, then the skh_temporal, skh_rectify, skh_rewind_guides, skh_moments and skh_denoise calls so far.
// on_rectify.bin: the skh_rectify_params of the last rectifying render() and, as a fifteenth word, the fast history's max_history.
#include "../../strelka_amd/host/oka_render.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace oka;

static bool dump(const std::string& dir, const std::string& name, const void* data, size_t bytes)
{
    FILE* f = fopen((dir + "/" + name).c_str(), "wb");
    if (!f)
        return false;
    const bool ok = fwrite(data, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

static const uint32_t W = 96, H = 64;
static const int FRAMES = 4;
static const bool MOVES[FRAMES] = { false, true, true, false };
static const uint32_t MOVED_INSTANCE = 1;

struct Session
{
    SettingsManager sm;
    SharedContext ctx;
    Scene scene;
    Render* render = nullptr;
    HipRender* hr = nullptr;
    Buffer* out = nullptr;
    bool open(const char* path)
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
        if (!hr->setTemporal(true))
            return false;
        hr->setInstanceMotion(true);
        return true;
    }
    bool sequence(const std::string& dir, const std::string& prefix)
    {
        FILE* calls = fopen((dir + "/" + prefix + "_calls.txt").c_str(), "w");
        if (!calls)
            return false;
        bool ok = true;
        for (int f = 0; f < FRAMES && ok; ++f)
        {
            scene.beginFrame();
            if (MOVES[f])
                scene.updateInstanceTransform(MOVED_INSTANCE, float4x4::translate(float3{ 0.1f, 0.05f, 0.0f }) * scene.getInstances()[MOVED_INSTANCE].transform);
            render->render(out);
            scene.endFrame();
            out->map();
            ok = dump(dir, prefix + "_" + std::to_string(f) + ".bin", out->getHostPointer(), (size_t)W * H * 16);
            skh_temporal_params tp;
            bool had = false;
            ok = ok && hr->temporalParams(tp, &had);
            skh_temporal_info ti = {};
            skh_rectify_info ri = {};
            skh_rewind_info wi = {};
            skh_moments_info mi = {};
            skh_denoise_info di = {};
            skh_get_temporal_info(hr->context(), &ti), skh_get_rectify_info(hr->context(), &ri), skh_get_rewind_info(hr->context(), &wi);
            skh_get_moments_info(hr->context(), &mi), skh_get_denoise_info(hr->context(), &di);
            fprintf(calls, "%d %llu %llu %llu %llu %llu\n", had ? 1 : 0, (unsigned long long)ti.calls, (unsigned long long)ri.calls, (unsigned long long)wi.calls,
                    (unsigned long long)mi.calls, (unsigned long long)di.calls);
        }
        fclose(calls);
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
        fprintf(stderr, "usage: hiprender_rectify_render <outdir> <scene.skscene>\n");
        return 2;
    }
    const std::string dir = argv[1];
    {
        Session plain;
        if (!plain.open(argv[2]))
            return 3;
        if (!plain.sequence(dir, "plain"))
            return 4;
        skh_rectify_params rp;
        if (plain.hr->rectifyParams(rp))
            return 6; // (none was handed over)
    }
    {
        Session off;
        if (!off.open(argv[2]))
            return 3;
        if (!off.hr->setHistoryRectification(true) || !off.hr->setHistoryRectification(false))
            return 5;
        if (!off.sequence(dir, "off"))
            return 4;
    }
    {
        Session guided;
        if (!guided.open(argv[2]))
            return 3;
        HipDenoise dn;
        dn.levels = 4, dn.sigmaColor = 0.2f;
        if (!guided.hr->setDenoiser(true, &dn) || !guided.hr->setVarianceGuidance(true) || !guided.hr->setHistoryRectification(true))
            return 5;
        if (!guided.sequence(dir, "ondn"))
            return 4;
    }
    Session on;
    if (!on.open(argv[2]))
        return 3;
    // refused settings leave the previous one (none) in force
    HipRectify bad;
    bad.radius = 4;
    if (on.hr->setHistoryRectification(true, &bad))
        return 7;
    bad = HipRectify(), bad.k = -1.0f;
    if (on.hr->setHistoryRectification(true, &bad))
        return 7;
    bad = HipRectify(), bad.fastHistory = 0.5f;
    if (on.hr->setHistoryRectification(true, &bad))
        return 7;
    if (!on.hr->setHistoryRectification(true))
        return 5;
    if (!on.sequence(dir, "on"))
        return 4;
    skh_rectify_params rp;
    float fast = 0.0f;
    if (!on.hr->rectifyParams(rp, &fast))
        return 8;
    uint32_t words[15];
    memcpy(words, &rp, 56), memcpy(words + 14, &fast, 4);
    if (!dump(dir, "on_rectify.bin", words, sizeof(words)))
        return 4;
    printf("hiprender_rectify_render ok\n");
    return 0;
}
