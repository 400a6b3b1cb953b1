// oka::HipRender::setDenoiser (the mirror build: strelka_amd/host/liboka_hip.so) behind hdRunner's frame loop:
//   hiprender_denoise <outdir> <scene.skscene> <frames>
// Three renderers on the same scene, <frames> frames each, every frame's output image (tonemapped, as map() hands it back) written out:
//   plain_<f>.bin   a HipRender that never heard of the denoiser
//   off_<f>.bin     one whose denoiser was turned on and off again before the first frame
//   dn_<f>.bin      one with the denoiser on (sigmaColor 0.2, four levels, the other defaults)
// The third one then moves its camera and renders two more frames.  counts.txt: skh_get_aov_info().calls of the three after <frames> frames (0, 0, 1: the guide
// planes are rendered once per accumulation), of the third after the camera move (2), and skh_get_denoise_info().calls of the third.  For the ctypes path to
// do the same: the scene arrays as the adapter uploaded them (the file names of strelka_amd/host/host_test.cpp), camera.bin, aov_params.bin (the guide pass's
// parameters) and denoise_params.bin (what render() handed to skh_denoise).
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
    bool frames(const std::string& dir, const char* prefix, int n)
    {
        for (int f = 0; f < n; ++f)
        {
            render->render(out);
            out->map();
            if (prefix && !dump(dir, std::string(prefix) + "_" + std::to_string(f) + ".bin", static_cast<const char*>(out->getHostPointer()), (size_t)W * H * 16))
                return false;
        }
        return true;
    }
    uint64_t aovCalls()
    {
        skh_aov_info info = {};
        skh_get_aov_info(hr->context(), &info);
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
    if (argc < 4)
    {
        fprintf(stderr, "usage: hiprender_denoise <outdir> <scene.skscene> <frames>\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int frames = atoi(argv[3]);
    unsigned long long counts[5] = {};
    {
        Session plain;
        if (!plain.open(argv[2]))
            return 3;
        if (!plain.frames(dir, "plain", frames))
            return 4;
        counts[0] = plain.aovCalls();
    }
    {
        Session off;
        if (!off.open(argv[2]))
            return 3;
        if (!off.hr->setDenoiser(true) || !off.hr->setDenoiser(false))
            return 5;
        if (!off.frames(dir, "off", frames))
            return 4;
        counts[1] = off.aovCalls();
        skh_denoise_info di = {};
        skh_get_denoise_info(off.hr->context(), &di);
        if (di.calls != 0 || di.scratch_bytes != 0)
            return 6;
    }
    Session dn;
    if (!dn.open(argv[2]))
        return 3;
    // a setting the library refuses is refused here, and the previous one stays
    HipDenoise bad;
    bad.levels = 9;
    if (dn.hr->setDenoiser(true, &bad) || dn.hr->lastError().empty())
        return 7;
    HipDenoise setting;
    setting.levels = 4, setting.sigmaColor = 0.2f;
    if (!dn.hr->setDenoiser(true, &setting))
        return 5;
    if (!dn.frames(dir, "dn", frames))
        return 4;
    counts[2] = dn.aovCalls();
    skh_denoise_params dp;
    skh_aov_params ap;
    if (!dn.hr->denoiseParams(dp) || !dn.hr->aovParams(ap, nullptr, false))
        return 8;
    // what the ctypes path needs (before the camera moves)
    Scene& scene = dn.scene;
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
    float mtx[32];
    memcpy(mtx, ap.view_to_world, 64), memcpy(mtx + 16, ap.clip_to_view, 64);
    if (!dump(dir, "vertices.bin", scene.getVertices().data(), scene.getVertices().size()) || !dump(dir, "indices.bin", scene.getIndices().data(), scene.getIndices().size()) ||
        !dump(dir, "meshes.bin", scene.getMeshes().data(), scene.getMeshes().size()) || !dump(dir, "lights.bin", scene.getLights().data(), scene.getLights().size()) ||
        !dump(dir, "instances.bin", inst.data(), inst.size()) || !dump(dir, "materials.bin", mats.data(), mats.size()) || !dump(dir, "camera.bin", mtx, 32) ||
        !dump(dir, "aov_params.bin", &ap, 1) || !dump(dir, "denoise_params.bin", &dp, 1))
        return 4;
    // a camera move restarts the accumulation: the guide planes are rendered once more, and only once
    Camera& cam = scene.getCamera(0);
    cam.setPosition(float3{ cam.position.x + 0.25f, cam.position.y, cam.position.z });
    if (!dn.frames(dir, nullptr, 2))
        return 4;
    counts[3] = dn.aovCalls();
    skh_denoise_info di = {};
    skh_get_denoise_info(dn.hr->context(), &di);
    counts[4] = di.calls;
    FILE* ft = fopen((dir + "/counts.txt").c_str(), "w");
    if (!ft)
        return 4;
    fprintf(ft, "%llu %llu %llu %llu %llu %zu\n", counts[0], counts[1], counts[2], counts[3], counts[4], dn.ctx.mSubframeIndex);
    fclose(ft);
    printf("hiprender_denoise ok\n");
    return 0;
}
