// oka::HipRender::setInstanceMotion (the mirror build: strelka_amd/host/liboka_hip.so) behind hdRunner's frame loop:
//   hiprender_motion <outdir> <scene.skscene>
// The sequence still, move-instance, move-instance, still (four frames; a move carries instance 1, the panel, by 0.1 in x and 0.05 in y through
// Scene::updateInstanceTransform), the camera at rest, every frame's output image (tonemapped, as map() hands it back) written out, by four renderers on the
// same scene, all with temporal accumulation on:
//   plain_<f>.bin   a HipRender that never heard of object motion
//   off_<f>.bin     one whose object motion was turned on and off again before the first frame
//   mo_<f>.bin      one with it on, the denoiser off
//   modn_<f>.bin    one with it on and the denoiser on (sigmaColor 0.2, four levels)
//   movg_<f>.bin    one with it on, that denoiser and variance guidance on (every default): skh_moments takes the rewound position too
// For the ctypes path to make the same calls, per frame of the last three (<p> = mo, modn, movg): <p>_aov_<f>.bin (the guide pass's skh_aov_params),
// <p>_temporal_<f>.bin (what render() handed to skh_temporal), <p>_instances_<f>.bin (the instance table of the frame) and a line of <p>_calls.txt:
// subframe_index enable_accumulation hadPrevious rewinds, the last the skh_rewind_guides calls so far.  Once: the scene arrays as the adapter uploaded them (the
// file names of strelka_amd/host/host_test.cpp) and denoise_params.bin; of movg also movg_variance_<f>.bin (what the frame's guided call handed to
// skh_denoise_variance; a frame that continues an accumulation repeats the one before).
// counts.txt: the skh_rewind_guides calls and the motion table's entries after the four frames of plain, off, mo, modn, movg.
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
static const int FRAMES = 4;
static const bool MOVES[FRAMES] = { false, true, true, false };
static const uint32_t MOVED_INSTANCE = 1;

static std::vector<skh_instance> instanceTable(Scene& scene)
{
    std::vector<skh_instance> inst(scene.getInstances().size());
    for (size_t i = 0; i < inst.size(); ++i)
    {
        const Instance& in = scene.getInstances()[i];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c)
                inst[i].transform[4 * r + c] = in.transform.m[c][r];
        inst[i].type = (uint32_t)in.type, inst[i].geom_id = in.mMeshId, inst[i].material_id = in.mMaterialId, inst[i].light_id = in.mLightId;
    }
    return inst;
}

struct Session
{
    SettingsManager sm;
    SharedContext ctx;
    Scene scene;
    Render* render = nullptr;
    HipRender* hr = nullptr;
    Buffer* out = nullptr;
    bool guided = false; // record what skh_denoise_variance got as well
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
        return hr->setTemporal(true);
    }
    skh_rewind_info rewindInfo()
    {
        skh_rewind_info info = {};
        skh_get_rewind_info(hr->context(), &info);
        return info;
    }
    // one frame; with `record`, what the ctypes path needs to repeat it
    bool frame(const std::string& dir, const std::string& prefix, int f, bool move, bool record, FILE* calls)
    {
        scene.beginFrame();
        if (move)
            scene.updateInstanceTransform(MOVED_INSTANCE, float4x4::translate(float3{ 0.1f, 0.05f, 0.0f }) * scene.getInstances()[MOVED_INSTANCE].transform);
        render->render(out);
        scene.endFrame();
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
        fprintf(calls, "%u %u %d %llu\n", index, accumulate, had ? 1 : 0, (unsigned long long)rewindInfo().calls);
        const std::vector<skh_instance> inst = instanceTable(scene);
        skh_vdenoise_params vp;
        if (guided && (!hr->varianceParams(vp) || !dump(dir, prefix + "_variance_" + std::to_string(f) + ".bin", &vp, 1)))
            return false;
        return dump(dir, prefix + "_aov_" + std::to_string(f) + ".bin", &ap, 1) && dump(dir, prefix + "_temporal_" + std::to_string(f) + ".bin", &tp, 1) &&
               dump(dir, prefix + "_instances_" + std::to_string(f) + ".bin", inst.data(), inst.size());
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
        fprintf(stderr, "usage: hiprender_motion <outdir> <scene.skscene>\n");
        return 2;
    }
    const std::string dir = argv[1];
    unsigned long long counts[10] = {};
    {
        Session plain;
        if (!plain.open(argv[2]))
            return 3;
        if (!plain.sequence(dir, "plain", false))
            return 4;
        counts[0] = plain.rewindInfo().calls, counts[1] = plain.rewindInfo().entries;
    }
    {
        Session off;
        if (!off.open(argv[2]))
            return 3;
        off.hr->setInstanceMotion(true);
        off.hr->setInstanceMotion(false);
        if (!off.sequence(dir, "off", false))
            return 4;
        counts[2] = off.rewindInfo().calls, counts[3] = off.rewindInfo().entries;
    }
    {
        Session both;
        if (!both.open(argv[2]))
            return 3;
        HipDenoise dn;
        dn.levels = 4, dn.sigmaColor = 0.2f;
        if (!both.hr->setDenoiser(true, &dn))
            return 5;
        both.hr->setInstanceMotion(true);
        if (!both.sequence(dir, "modn", true))
            return 4;
        skh_denoise_params dp;
        if (!both.hr->denoiseParams(dp) || !dump(dir, "denoise_params.bin", &dp, 1))
            return 8;
        counts[6] = both.rewindInfo().calls, counts[7] = both.rewindInfo().entries;
    }
    {
        Session vg;
        if (!vg.open(argv[2]))
            return 3;
        HipDenoise dn;
        dn.levels = 4, dn.sigmaColor = 0.2f;
        if (!vg.hr->setDenoiser(true, &dn) || !vg.hr->setVarianceGuidance(true))
            return 5;
        vg.hr->setInstanceMotion(true);
        vg.guided = true;
        if (!vg.sequence(dir, "movg", true))
            return 4;
        counts[8] = vg.rewindInfo().calls, counts[9] = vg.rewindInfo().entries;
    }
    Session mo;
    if (!mo.open(argv[2]))
        return 3;
    mo.hr->setInstanceMotion(true);
    // what the ctypes path needs: the scene as uploaded
    Scene& scene = mo.scene;
    const std::vector<skh_instance> inst = instanceTable(scene);
    std::vector<skh_material> mats;
    for (auto& m : scene.getMaterials())
        mats.push_back(m.args);
    if (!mo.sequence(dir, "mo", true))
        return 4;
    skh_aov_params ap;
    if (!mo.hr->aovParams(ap, nullptr, false))
        return 8;
    float mtx[32];
    memcpy(mtx, ap.view_to_world, 64), memcpy(mtx + 16, ap.clip_to_view, 64);
    if (!dump(dir, "vertices.bin", scene.getVertices().data(), scene.getVertices().size()) || !dump(dir, "indices.bin", scene.getIndices().data(), scene.getIndices().size()) ||
        !dump(dir, "meshes.bin", scene.getMeshes().data(), scene.getMeshes().size()) || !dump(dir, "lights.bin", scene.getLights().data(), scene.getLights().size()) ||
        !dump(dir, "instances.bin", inst.data(), inst.size()) || !dump(dir, "materials.bin", mats.data(), mats.size()) || !dump(dir, "camera.bin", mtx, 32))
        return 4;
    counts[4] = mo.rewindInfo().calls, counts[5] = mo.rewindInfo().entries;
    FILE* ft = fopen((dir + "/counts.txt").c_str(), "w");
    if (!ft)
        return 4;
    for (unsigned long long c : counts)
        fprintf(ft, "%llu ", c);
    fprintf(ft, "\n");
    fclose(ft);
    printf("hiprender_motion ok\n");
    return 0;
}
