// oka::HipRender (the mirror build: strelka_amd/host/liboka_hip.so) driven like hdRunner's frame loop through an instance move:
//   hiprender_move <outdir> <scene.skscene> <framesBefore> <framesAfter>
// renders framesBefore frames, moves instance 1 with Scene::updateInstanceTransform (the reference's edit channel, scene.cpp:445-450),
// renders framesAfter frames, and writes what the ctypes path needs to render the same: the arrays of the MOVED scene as the adapter uploads them
// (the file names of strelka_amd/host/host_test.cpp: vertices.bin ... instances.bin, camera.bin), the accumulation (accum.bin) and the frame
// bookkeeping (frames.txt: mSubframeIndex, mFrameNumber, the dirty-set size the adapter left behind, skh_build_info.refit).
#include "../../strelka_amd/host/oka_render.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace oka;

template <typename T>
static bool dump(const std::string& dir, const char* name, const T* data, size_t n)
{
    FILE* f = fopen((dir + "/" + name).c_str(), "wb");
    if (!f)
        return false;
    const bool ok = fwrite(data, sizeof(T), n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv)
{
    if (argc < 5)
    {
        fprintf(stderr, "usage: hiprender_move <outdir> <scene.skscene> <framesBefore> <framesAfter>\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int before = atoi(argv[3]), after = atoi(argv[4]);
    Scene scene;
    if (!scene.loadDump(argv[2]) || scene.getInstances().size() < 2)
        return 3;
    const uint32_t W = 96, H = 64;
    // hdRunner defaults (src/hdRunner/main.cpp:510-542), accumulation over more samples than the loop renders
    SettingsManager sm;
    SharedContext ctx;
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
    Render* render = RenderFactory::createRender(RenderType::eCompute);
    render->setSharedContext(&ctx);
    ctx.mRender = render;
    render->setScene(&scene);
    render->init();
    HipRender* hr = static_cast<HipRender*>(render);
    Buffer* out = render->createBuffer(BufferDesc{ W, H, BufferFormat::FLOAT4 });
    for (int f = 0; f < before; ++f)
    {
        render->render(out);
        out->map();
    }
    // the panel turns a little and slides along the floor
    const float4x4 moved = float4x4::translate(float3{ -0.5f, 0.0f, 0.35f }) * scene.getInstances()[1].transform *
                           float4x4::fromQuat(quatFromEulerRadians(float3{ 0.0f, 0.45f, 0.0f }));
    scene.updateInstanceTransform(1, moved);
    for (int f = 0; f < after; ++f)
    {
        render->render(out);
        out->map();
    }
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
    // the camera as render() hands it over (a camera restored from a dump is re-derived from its view matrix: its bits are its own)
    Camera& cam = scene.getCamera(0);
    float mtx[32];
    const float4x4 v2w = cam.matrices.view.inverse();
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
        {
            mtx[4 * r + c] = v2w.m[c][r];
            mtx[16 + 4 * r + c] = cam.matrices.invPerspective.m[c][r];
        }
    std::vector<float> accum((size_t)W * H * 4);
    skh_read_accum(hr->context(), accum.data());
    skh_build_info bi;
    if (skh_get_build_info(hr->context(), &bi) != SKH_OK)
        return 6;
    if (!dump(dir, "vertices.bin", scene.getVertices().data(), scene.getVertices().size()) || !dump(dir, "indices.bin", scene.getIndices().data(), scene.getIndices().size()) ||
        !dump(dir, "meshes.bin", scene.getMeshes().data(), scene.getMeshes().size()) || !dump(dir, "lights.bin", scene.getLights().data(), scene.getLights().size()) ||
        !dump(dir, "instances.bin", inst.data(), inst.size()) || !dump(dir, "materials.bin", mats.data(), mats.size()) || !dump(dir, "camera.bin", mtx, 32) ||
        !dump(dir, "accum.bin", accum.data(), accum.size()))
        return 4;
    FILE* ft = fopen((dir + "/frames.txt").c_str(), "w");
    if (!ft)
        return 4;
    fprintf(ft, "%zu %zu %zu %u\n", ctx.mSubframeIndex, ctx.mFrameNumber, scene.getDirtyInstances().size(), bi.refit);
    fclose(ft);
    if (!hr->lastError().empty())
    {
        fprintf(stderr, "%s\n", hr->lastError().c_str());
        return 5;
    }
    delete out;
    delete render;
    printf("hiprender_move ok\n");
    return 0;
}
