// oka::HipRender::setTemporal (the mirror build: strelka_amd/host/liboka_hip.so) behind hdRunner's frame loop:
//   hiprender_temporal <outdir> <scene.skscene>
// The sequence still, still, move, move, still (five frames; a move shifts the camera by 0.1 in x), every frame's output image (tonemapped, as map() hands it
// back) written out, by four renderers on the same scene:
//   plain_<f>.bin   a HipRender that never heard of the feature
//   off_<f>.bin     one whose temporal accumulation was turned on and off again before the first frame
//   tp_<f>.bin      one with it on (every default), the denoiser off
//   tpdn_<f>.bin    one with it on and the denoiser on (sigmaColor 0.2, four levels)
// For the ctypes path to make the same calls, per frame of the third and fourth (<p> = tp, tpdn): <p>_aov_<f>.bin (the skh_aov_params of the frame's camera: the
// guide pass's), <p>_temporal_<f>.bin (what render() handed to skh_temporal) and a line of <p>_calls.txt: subframe_index enable_accumulation hadPrevious.  Once: the scene arrays as the
// adapter uploaded them (the file names of strelka_amd/host/host_test.cpp) and denoise_params.bin.
// counts.txt, of the third renderer: guide passes and skh_temporal calls after the five frames; then, after setEnvironment and one more frame, both again and
// whether that frame's call had a previous frame (the history was dropped: 0); of the first two renderers: guide passes and skh_temporal calls (0 0 0 0).
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
        return true;
    }
    // one frame; with `record`, what the ctypes path needs to repeat it
    bool frame(const std::string& dir, const std::string& prefix, int f, bool move, bool record, FILE* calls)
    {
        if (move)
        {
            Camera& cam = scene.getCamera(0);
            cam.setPosition(float3{ cam.position.x + 0.1f, cam.position.y, cam.position.z });
        }
        render->render(out);
        out->map();
        if (!dump(dir, prefix + "_" + std::to_string(f) + ".bin", static_cast<const char*>(out->getHostPointer()), (size_t)W * H * 16))
            return false;
        if (!record)
            return true;
        skh_aov_params ap;
        skh_temporal_params tp;
        bool had = false;
        uint32_t index = 0, accumulate = 0;
        if (!hr->aovParams(ap, nullptr, false) || !hr->temporalParams(tp, &had))
            return false;
        hr->lastSample(index, accumulate);
        fprintf(calls, "%u %u %d\n", index, accumulate, had ? 1 : 0);
        return dump(dir, prefix + "_aov_" + std::to_string(f) + ".bin", &ap, 1) && dump(dir, prefix + "_temporal_" + std::to_string(f) + ".bin", &tp, 1);
    }
    bool sequence(const std::string& dir, const std::string& prefix, bool record)
    {
        FILE* calls = record ? fopen((dir + "/" + prefix + "_calls.txt").c_str(), "w") : nullptr;
        if (record && !calls)
            return false;
        bool ok = true;
        for (int f = 0; f < FRAMES && ok; ++f)
            ok = frame(dir, prefix, f, MOVES[f], record, calls);
        if (calls)
            fclose(calls);
        return ok;
    }
    unsigned long long aovCalls()
    {
        skh_aov_info info = {};
        skh_get_aov_info(hr->context(), &info);
        return info.calls;
    }
    unsigned long long temporalCalls()
    {
        skh_temporal_info info = {};
        skh_get_temporal_info(hr->context(), &info);
        return info.calls;
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
        fprintf(stderr, "usage: hiprender_temporal <outdir> <scene.skscene>\n");
        return 2;
    }
    const std::string dir = argv[1];
    unsigned long long counts[9] = {};
    {
        Session plain;
        if (!plain.open(argv[2]))
            return 3;
        if (!plain.sequence(dir, "plain", false))
            return 4;
        counts[5] = plain.aovCalls(), counts[6] = plain.temporalCalls();
    }
    {
        Session off;
        if (!off.open(argv[2]))
            return 3;
        if (!off.hr->setTemporal(true) || !off.hr->setTemporal(false))
            return 5;
        if (!off.sequence(dir, "off", false))
            return 4;
        counts[7] = off.aovCalls(), counts[8] = off.temporalCalls();
    }
    {
        Session both;
        if (!both.open(argv[2]))
            return 3;
        HipDenoise dn;
        dn.levels = 4, dn.sigmaColor = 0.2f;
        if (!both.hr->setDenoiser(true, &dn) || !both.hr->setTemporal(true))
            return 5;
        if (!both.sequence(dir, "tpdn", true))
            return 4;
        skh_denoise_params dp;
        if (!both.hr->denoiseParams(dp) || !dump(dir, "denoise_params.bin", &dp, 1))
            return 8;
    }
    Session tp;
    if (!tp.open(argv[2]))
        return 3;
    // a setting the library refuses is refused here, and the previous one stays
    HipTemporal bad;
    bad.normalMin = 1.5f;
    if (tp.hr->setTemporal(true, &bad) || tp.hr->lastError().empty())
        return 7;
    if (!tp.hr->setTemporal(true))
        return 5;
    // what the ctypes path needs: the scene as uploaded
    Scene& scene = tp.scene;
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
    if (!tp.sequence(dir, "tp", true))
        return 4;
    skh_aov_params ap;
    if (!tp.hr->aovParams(ap, nullptr, false))
        return 8;
    float mtx[32];
    memcpy(mtx, ap.view_to_world, 64), memcpy(mtx + 16, ap.clip_to_view, 64);
    if (!dump(dir, "vertices.bin", scene.getVertices().data(), scene.getVertices().size()) || !dump(dir, "indices.bin", scene.getIndices().data(), scene.getIndices().size()) ||
        !dump(dir, "meshes.bin", scene.getMeshes().data(), scene.getMeshes().size()) || !dump(dir, "lights.bin", scene.getLights().data(), scene.getLights().size()) ||
        !dump(dir, "instances.bin", inst.data(), inst.size()) || !dump(dir, "materials.bin", mats.data(), mats.size()) || !dump(dir, "camera.bin", mtx, 32))
        return 4;
    counts[0] = tp.aovCalls(), counts[1] = tp.temporalCalls();
    // a new sky drops the history: the next call has no previous frame
    const float sky[4 * 2 * 3] = { 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f,
                                   0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f };
    const float scale[3] = { 1.0f, 1.0f, 1.0f };
    if (!tp.hr->setEnvironment(sky, 4, 2, scale))
        return 9;
    tp.render->render(tp.out);
    skh_temporal_params last;
    bool had = true;
    if (!tp.hr->temporalParams(last, &had))
        return 8;
    counts[2] = tp.aovCalls(), counts[3] = tp.temporalCalls(), counts[4] = had ? 1 : 0;
    FILE* ft = fopen((dir + "/counts.txt").c_str(), "w");
    if (!ft)
        return 4;
    for (unsigned long long c : counts)
        fprintf(ft, "%llu ", c);
    fprintf(ft, "%zu\n", tp.ctx.mSubframeIndex);
    fclose(ft);
    printf("hiprender_temporal ok\n");
    return 0;
}
