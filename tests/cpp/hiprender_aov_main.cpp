// oka::HipRender::renderAovs / pick (the mirror build: strelka_amd/host/liboka_hip.so) behind hdRunner's frame loop:
//   hiprender_aov <outdir> <scene.skscene> <frames>
// renders <frames> frames, asks for all seven first-hit planes -- through the pixel centres (centre_<k>.bin) and for sample 0 (sample0_<k>.bin) --, for planes
// ids | normal of the region {5, 3, 17, 11} (region_0.bin, region_2.bin), picks the first pixel of each kind the ids plane shows (picks.bin: x, y and the 28 words of
// HipPick's planes, per pick), renders one more frame, and writes what the ctypes path needs to do the same: the scene arrays as the adapter uploaded them (the file
// names of strelka_amd/host/host_test.cpp), the parameters renderAovs built (aov_params.bin: skh_aov_params, pixel centre, whole image) and the accumulation
// (accum.bin) with the frame bookkeeping (frames.txt: mSubframeIndex, mFrameNumber).
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

int main(int argc, char** argv)
{
    if (argc < 4)
    {
        fprintf(stderr, "usage: hiprender_aov <outdir> <scene.skscene> <frames>\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int frames = atoi(argv[3]);
    Scene scene;
    if (!scene.loadDump(argv[2]))
        return 3;
    const uint32_t W = 96, H = 64;
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
    // before the first render() there is neither a scene nor an image on the device: refused, not crashed
    Buffer* none[SKH_AOV_COUNT] = {};
    if (hr->renderAovs(1u, none) || hr->lastError().empty())
        return 7;
    for (int f = 0; f < frames; ++f)
    {
        render->render(out);
        out->map();
    }
    Buffer* planes[SKH_AOV_COUNT];
    for (uint32_t k = 0; k < SKH_AOV_COUNT; ++k)
        planes[k] = render->createBuffer(BufferDesc{ W, H, BufferFormat::FLOAT4 });
    const uint32_t all = (1u << SKH_AOV_COUNT) - 1u;
    std::vector<uint32_t> ids;
    for (int mode = 0; mode < 2; ++mode)
    {
        if (!hr->renderAovs(all, planes, nullptr, mode == 1))
            return 8;
        for (uint32_t k = 0; k < SKH_AOV_COUNT; ++k)
        {
            planes[k]->map();
            if (!dump(dir, std::string(mode ? "sample0_" : "centre_") + std::to_string(k) + ".bin", static_cast<const char*>(planes[k]->getHostPointer()), (size_t)W * H * 16))
                return 4;
            if (mode == 0 && k == SKH_AOV_IDS)
            {
                ids.resize((size_t)W * H * 4);
                memcpy(ids.data(), planes[k]->getHostPointer(), ids.size() * 4);
            }
        }
    }
    // a region, two planes; a buffer that is too small is refused
    const uint32_t region[4] = { 5, 3, 17, 11 };
    Buffer* small[SKH_AOV_COUNT] = {};
    small[SKH_AOV_IDS] = render->createBuffer(BufferDesc{ 17, 11, BufferFormat::FLOAT4 });
    small[SKH_AOV_NORMAL] = render->createBuffer(BufferDesc{ 17, 11, BufferFormat::FLOAT4 });
    if (!hr->renderAovs((1u << SKH_AOV_IDS) | (1u << SKH_AOV_NORMAL), small, region))
        return 8;
    for (uint32_t k : { SKH_AOV_IDS, SKH_AOV_NORMAL })
    {
        small[k]->map();
        if (!dump(dir, "region_" + std::to_string(k) + ".bin", static_cast<const char*>(small[k]->getHostPointer()), (size_t)17 * 11 * 16))
            return 4;
    }
    if (hr->renderAovs(1u << SKH_AOV_IDS, small))
        return 9; // (17 x 11 words for the whole image)
    // pick: the first pixel of every kind in the image
    std::vector<uint32_t> picks;
    for (uint32_t kind = 0; kind < 4; ++kind)
        for (uint32_t i = 0; i < W * H; ++i)
            if (ids[4 * (size_t)i + 3] == kind)
            {
                HipPick pk;
                if (!hr->pick(i % W, i / W, pk))
                    return 10;
                uint32_t w[28] = { pk.instanceId, pk.primId, pk.material, pk.kind };
                const float f[24] = { pk.t, pk.u, pk.v, pk.depth, pk.normal[0], pk.normal[1], pk.normal[2], pk.facing, pk.position[0], pk.position[1], pk.position[2],
                                      pk.kind ? 1.0f : 0.0f, pk.geomNormal[0], pk.geomNormal[1], pk.geomNormal[2], 0.0f, pk.albedo[0], pk.albedo[1], pk.albedo[2],
                                      pk.kind ? 1.0f : 0.0f, pk.texcoord[0], pk.texcoord[1], 0.0f, 0.0f };
                memcpy(w + 4, f, sizeof(f));
                picks.push_back(i % W), picks.push_back(i / W);
                picks.insert(picks.end(), w, w + 28);
                break;
            }
    HipPick outside;
    if (hr->pick(W, 0, outside))
        return 11;
    skh_aov_params ap;
    if (!hr->aovParams(ap, nullptr, false))
        return 12;
    render->render(out); // the frame goes on as if nothing had happened
    out->map();
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
    std::vector<float> accum((size_t)W * H * 4);
    skh_read_accum(hr->context(), accum.data());
    if (!dump(dir, "vertices.bin", scene.getVertices().data(), scene.getVertices().size()) || !dump(dir, "indices.bin", scene.getIndices().data(), scene.getIndices().size()) ||
        !dump(dir, "meshes.bin", scene.getMeshes().data(), scene.getMeshes().size()) || !dump(dir, "lights.bin", scene.getLights().data(), scene.getLights().size()) ||
        !dump(dir, "instances.bin", inst.data(), inst.size()) || !dump(dir, "materials.bin", mats.data(), mats.size()) || !dump(dir, "camera.bin", mtx, 32) ||
        !dump(dir, "aov_params.bin", &ap, 1) || !dump(dir, "picks.bin", picks.data(), picks.size()) || !dump(dir, "accum.bin", accum.data(), accum.size()))
        return 4;
    FILE* ft = fopen((dir + "/frames.txt").c_str(), "w");
    if (!ft)
        return 4;
    fprintf(ft, "%zu %zu\n", ctx.mSubframeIndex, ctx.mFrameNumber);
    fclose(ft);
    for (Buffer* b : planes)
        delete b;
    delete small[SKH_AOV_IDS];
    delete small[SKH_AOV_NORMAL];
    delete out;
    delete render;
    printf("hiprender_aov ok\n");
    return 0;
}
