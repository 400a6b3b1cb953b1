// oka::HipBuffer / oka::HipRender: Strelka's render interface implemented on the C ABI of libstrelka_hip.so -- see HipRender.h.
// Plain C++17 host code (no HIP headers): every device operation goes through include/strelka_hip.h.  render() follows
// OptiXRender::render (src/render/optix/OptixRender.cpp:874-1057) statement by statement: the reset rules, the exposure formula, the
// sub-frame bookkeeping and the hand-back after the last sample are the adapter's contract.
#include "HipRender.h"
#ifdef SKH_WITH_STRELKA_HEADERS
#    include "SkhMaterials.h"

// The reference's texture loader (OptixRender.cpp:18,1191-1264).  In the reference STB_IMAGE_STATIC + STB_IMAGE_IMPLEMENTATION sit in OptixRender.cpp:16-17, which
// strelka_hip.cmake drops from the render target: this file fills that slot, so that targets which link `render` without the scene loader
// (HdStrelka: render + scene + materialmanager) still resolve stbi_load / stbi_image_free.
#    define STB_IMAGE_STATIC // (as OptixRender.cpp:16: the symbols stay file-local, gltfloader.cpp:5 has its own copy)
#    define STB_IMAGE_IMPLEMENTATION
#    include <stb_image.h>
#    include <filesystem>
#endif

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>

namespace oka
{

// the scene's instances as skh_set_instances / skh_update_accel take them
static std::vector<skh_instance> instanceTable(Scene& sc)
{
    std::vector<skh_instance> inst(sc.getInstances().size());
    for (size_t i = 0; i < inst.size(); ++i)
    {
        const Instance& in = sc.getInstances()[i];
        // glm::float3x4(glm::rowMajor4(transform)) (OptixRender.cpp:438): rows of the affine transform
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c)
                inst[i].transform[4 * r + c] = in.transform[c][r];
        inst[i].type = (uint32_t)in.type;
        inst[i].geom_id = in.mMeshId;
        inst[i].material_id = in.mMaterialId;
        inst[i].light_id = in.mLightId;
    }
    return inst;
}

HipBuffer::HipBuffer(skh_context* ctx, void* devicePtr, BufferFormat format, uint32_t width, uint32_t height) : mCtx(ctx), mDeviceData(devicePtr)
{
    mFormat = format;
    mWidth = width;
    mHeight = height;
}
HipBuffer::~HipBuffer()
{
    if (mRegistered)
        skh_host_unregister(mCtx, mRegistered);
    if (mDeviceData)
        skh_buffer_free(mCtx, mDeviceData);
}
void HipBuffer::resize(uint32_t width, uint32_t height)
{
    if (mDeviceData)
        skh_buffer_free(mCtx, mDeviceData);
    mDeviceData = nullptr;
    mWidth = width;
    mHeight = height;
    skh_buffer_alloc(mCtx, (size_t)mWidth * mHeight * getElementSize(), &mDeviceData);
}
void* HipBuffer::map()
{
    const size_t bytes = (size_t)mWidth * mHeight * getElementSize();
    if (mHostData.size() != bytes || mRegistered != mHostData.data())
    {
        // the host mirror is the reference's std::vector (buffer.h:60-88); page-locked once per size so that the copy the caller
        // asks for after EVERY sub-frame (RenderPass.cpp:441-447) runs at PCIe rate instead of through a staging buffer
        if (mRegistered)
            skh_host_unregister(mCtx, mRegistered);
        mRegistered = nullptr;
        mHostData.resize(bytes);
        if (bytes && skh_host_register(mCtx, mHostData.data(), bytes) == SKH_OK)
            mRegistered = mHostData.data();
    }
    skh_buffer_download(mCtx, mDeviceData, mHostData.data(), bytes);
    return nullptr;
}

HipRender::~HipRender()
{
    freeGuides();
    if (mCtx && mGatherBuf)
        skh_buffer_free(mCtx, mGatherBuf);
    if (mCtx)
        skh_destroy(mCtx);
}

bool HipRender::enableTileSharing(const void* commId, int worldSize, int rank, uint32_t tileSize)
{
    if (!mCtx || worldSize < 1 || rank < 0 || rank >= worldSize)
        return false;
    if (worldSize > 1 && !check(skh_comm_init(mCtx, commId, worldSize, rank), "skh_comm_init"))
        return false;
    mSharing = true; // (world size 1 keeps the whole path -- tile set, gather, scatter -- minus the sends: what a 1-GPU box can test)
    mWorld = worldSize;
    mRank = rank;
    mTileSize = tileSize;
    mWidth = mHeight = 0; // the next render() re-derives the tile share
    return true;
}

// tiles t = rank (mod world) of the row-major tile list: interleaving spreads expensive image regions over the GPUs
bool HipRender::applyTiles(uint32_t width, uint32_t height)
{
    if (!mSharing)
        return true;
    std::vector<std::vector<uint32_t>> perRank(mWorld);
    uint32_t t = 0;
    for (uint32_t y = 0; y < height; y += mTileSize)
        for (uint32_t x = 0; x < width; x += mTileSize, ++t)
        {
            perRank[t % mWorld].push_back(x);
            perRank[t % mWorld].push_back(y);
        }
    mMaxTiles = (t + mWorld - 1) / mWorld;
    const std::vector<uint32_t>& mine = perRank[mRank];
    if (!check(skh_set_tiles(mCtx, mTileSize, mine.data(), (uint32_t)(mine.size() / 2)), "skh_set_tiles"))
        return false;
    if (mRank == 0)
    {
        // padding tiles get an origin outside the image: skh_scatter_tiles drops them
        mAllTileXY.assign((size_t)mWorld * mMaxTiles * 2, std::max(width, height));
        for (int r = 0; r < mWorld; ++r)
            std::copy(perRank[r].begin(), perRank[r].end(), mAllTileXY.begin() + (size_t)r * mMaxTiles * 2);
        if (mGatherBuf)
            skh_buffer_free(mCtx, mGatherBuf);
        mGatherBuf = nullptr;
        return check(skh_buffer_alloc(mCtx, (size_t)mWorld * mMaxTiles * mTileSize * mTileSize * 16, &mGatherBuf), "skh_buffer_alloc");
    }
    return true;
}
bool HipRender::check(skh_status s, const char* what)
{
    if (s == SKH_OK)
        return true;
    // reference behaviour: log + assert(0), keep going in release builds (OptixRender.cpp:61-103)
    mError = std::string(what) + ": " + (mCtx ? skh_last_error(mCtx) : "no context");
    std::cerr << "[HipRender] " << mError << std::endl;
    assert(0);
    return false;
}
void HipRender::init()
{
    int device = 0;
    if (const char* lr = getenv("LOCAL_RANK"))
        device = atoi(lr);
    check(skh_create(device, &mCtx), "skh_create");
}
Buffer* HipRender::createBuffer(const BufferDesc& desc)
{
    assert(desc.format == BufferFormat::FLOAT4); // OptixRender.cpp:1109
    void* d = nullptr;
    if (!check(skh_buffer_alloc(mCtx, (size_t)desc.width * desc.height * Buffer::getElementSize(desc.format), &d), "skh_buffer_alloc"))
        return nullptr;
    return new HipBuffer(mCtx, d, desc.format, desc.width, desc.height);
}
void HipRender::uploadScene()
{
    Scene& sc = *mScene;
    static_assert(sizeof(Scene::Vertex) == sizeof(skh_vertex) && sizeof(Mesh) == sizeof(skh_mesh) && sizeof(Curve) == sizeof(skh_curve), "layouts");
    static_assert(sizeof(Scene::Light) == sizeof(skh_light), "light layout");
    check(skh_set_geometry(mCtx, reinterpret_cast<const skh_vertex*>(sc.getVertices().data()), (uint32_t)sc.getVertices().size(),
                           sc.getIndices().data(), (uint32_t)sc.getIndices().size(),
                           reinterpret_cast<const skh_mesh*>(sc.getMeshes().data()), (uint32_t)sc.getMeshes().size()),
          "skh_set_geometry");
    if (!sc.getCurves().empty())
        check(skh_set_curves(mCtx, reinterpret_cast<const float*>(sc.getCurvesPoint().data()), (uint32_t)sc.getCurvesPoint().size(),
                             sc.getCurvesWidths().data(), (uint32_t)sc.getCurvesWidths().size(), sc.getCurvesVertexCounts().data(),
                             (uint32_t)sc.getCurvesVertexCounts().size(), reinterpret_cast<const skh_curve*>(sc.getCurves().data()),
                             (uint32_t)sc.getCurves().size()),
              "skh_set_curves");
    std::vector<skh_instance> inst = instanceTable(sc);
    check(skh_set_instances(mCtx, inst.data(), (uint32_t)inst.size()), "skh_set_instances");
    mSentInstances = inst;
    measureScene(inst);
    check(skh_set_lights(mCtx, reinterpret_cast<const skh_light*>(sc.getLights().data()), (uint32_t)sc.getLights().size()), "skh_set_lights");
    mLightsUploaded = true;
    applyLightShapes(); // (the table is indexed as the light list is: it follows every upload of the list)
    uploadMaterials();
    check(skh_build_accel(mCtx, SKH_BUILD_LBVH), "skh_build_accel");
}

bool HipRender::sendMovedInstances()
{
    Scene& sc = *mScene;
    const std::vector<skh_instance> inst = instanceTable(sc);
    bool moved = false;
    for (uint32_t id : sc.getDirtyInstances())
        moved = moved || (id < inst.size() && id < mSentInstances.size() &&
                          memcmp(inst[id].transform, mSentInstances[id].transform, sizeof(inst[id].transform)) != 0);
    if (!moved)
        return false;
    // (the caller's dirty set is left alone: it belongs to the scene's frame protocol, beginFrame / endFrame)
    check(skh_update_accel(mCtx, inst.data(), (uint32_t)inst.size()), "skh_update_accel");
    mSentInstances = inst;
    measureScene(inst);
    return true;
}

// the diagonal of the world-space box around the mesh instances (each mesh's own box under its instance's transform): the denoiser's default sigmaPlane is a
// fraction of it
void HipRender::measureScene(const std::vector<skh_instance>& inst)
{
    Scene& sc = *mScene;
    const auto& verts = sc.getVertices();
    const auto& meshes = sc.getMeshes();
    std::vector<double> box(6 * meshes.size());
    std::vector<char> have(meshes.size(), 0);
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (const skh_instance& in : inst)
    {
        if (in.type != SKH_INSTANCE_MESH || in.geom_id >= meshes.size())
            continue;
        const skh_mesh& m = reinterpret_cast<const skh_mesh&>(meshes[in.geom_id]);
        if (m.vertex_count == 0u || (size_t)m.vertex_offset + m.vertex_count > verts.size())
            continue;
        double* b = &box[6 * (size_t)in.geom_id];
        if (!have[in.geom_id])
        {
            have[in.geom_id] = 1;
            for (int k = 0; k < 3; ++k)
                b[k] = INFINITY, b[3 + k] = -INFINITY;
            for (uint32_t v = 0; v < m.vertex_count; ++v)
            {
                const float* pos = reinterpret_cast<const skh_vertex&>(verts[m.vertex_offset + v]).pos;
                for (int k = 0; k < 3; ++k)
                    b[k] = std::min(b[k], (double)pos[k]), b[3 + k] = std::max(b[3 + k], (double)pos[k]);
            }
        }
        for (int corner = 0; corner < 8; ++corner)
        {
            const double p[3] = { b[(corner & 1) ? 3 : 0], b[(corner & 2) ? 4 : 1], b[(corner & 4) ? 5 : 2] };
            for (int r = 0; r < 3; ++r)
            {
                const double w = in.transform[4 * r] * p[0] + in.transform[4 * r + 1] * p[1] + in.transform[4 * r + 2] * p[2] + in.transform[4 * r + 3];
                lo[r] = std::min(lo[r], w), hi[r] = std::max(hi[r], w);
            }
        }
    }
    double d2 = 0.0;
    for (int k = 0; k < 3; ++k)
        d2 += hi[k] >= lo[k] ? (hi[k] - lo[k]) * (hi[k] - lo[k]) : 0.0;
    mSceneDiagonal = (float)std::sqrt(d2);
}

void HipRender::freeGuides()
{
    for (void*& g : mGuide)
    {
        if (mCtx && g)
            skh_buffer_free(mCtx, g);
        g = nullptr;
    }
    for (void** g : { &mPrevGuide[0], &mPrevGuide[1], &mPrevGuide[2], &mHistory[0], &mHistory[1], &mVarianceImage, &mMotion, &mMoments[0], &mMoments[1],
                      &mRewound[0], &mRewound[1], &mFast[0], &mFast[1], &mRectifyImage })
    {
        if (mCtx && *g)
            skh_buffer_free(mCtx, *g);
        *g = nullptr;
    }
    mGuideWidth = mGuideHeight = 0;
    mGuidesValid = mPrevGuidesValid = mHistoryValid = mMomentsValid = mFastValid = false;
}

bool HipRender::setDenoiser(bool on, const HipDenoise* params)
{
    if (!on)
    {
        mDenoise = false;
        if (!mTemporal)
            freeGuides();
        memset(&mDenoiseApplied, 0, sizeof(mDenoiseApplied));
        return !mCtx || check(skh_denoise(mCtx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "skh_denoise"); // (the library's scratch goes too)
    }
    const HipDenoise d = params ? *params : HipDenoise();
    // (checked here with an image, an exposure and a scene that pass: the real ones are render()'s)
    const float one[3] = { 1.0f, 1.0f, 1.0f };
    const skh_denoise_params probe = hipDenoiseParams(d, 1u, 1u, one, 1.0f);
    if (skh_denoise_check(&probe) != SKH_OK)
    {
        mError = "setDenoiser: the setting was refused (levels 1 .. 8, finite positive sigmas and floor)";
        return false;
    }
    mDenoise = true;
    mDenoiseSetting = d;
    return true;
}

bool HipRender::setTemporal(bool on, const HipTemporal* params)
{
    const HipTemporal t = params ? *params : HipTemporal();
    // (checked here with an image and a scene that pass: the real ones are render()'s)
    const skh_temporal_params probe = hipTemporalParams(t, 1u, 1u, nullptr, 1.0f, 1.0f);
    if (on && skh_temporal_check(&probe) != SKH_OK)
    {
        mError = "setTemporal: the setting was refused (normalMin in [-1, 1], a positive tolerance, finite maxHistory >= 1 and positive floor)";
        return false;
    }
    dropHistory(); // (a history kept under another setting is not this one's)
    mPrevGuidesValid = false;
    memset(&mTemporalApplied, 0, sizeof(mTemporalApplied));
    if (!on)
    {
        mTemporal = false;
        if (!mDenoise)
            freeGuides();
        return true;
    }
    if (!mTemporal)
        mGuidesValid = false; // (the buffers this feature adds come with the next guide pass)
    mTemporal = true;
    mTemporalSetting = t;
    return true;
}

bool HipRender::setVarianceGuidance(bool on, const HipVariance* params)
{
    const HipVariance v = params ? *params : HipVariance();
    // (checked here with an image, an exposure and a scene that pass: the real ones are render()'s)
    const float one[3] = { 1.0f, 1.0f, 1.0f };
    const skh_vdenoise_params probe = hipVarianceParams(v, HipDenoise(), 1u, 1u, one, 1.0f);
    if (on && skh_vdenoise_check(&probe) != SKH_OK)
    {
        mError = "setVarianceGuidance: the setting was refused (a positive sigmaLuminance, finite positive epsilon, finite minHistory >= 1)";
        return false;
    }
    mMomentsValid = false; // (moments kept under another setting are not this one's)
    memset(&mVarianceApplied, 0, sizeof(mVarianceApplied));
    mVariance = on;
    if (on)
        mVarianceSetting = v;
    else
        for (void** g : { &mVarianceImage, &mMotion, &mMoments[0], &mMoments[1] })
        {
            if (mCtx && *g)
                skh_buffer_free(mCtx, *g);
            *g = nullptr;
        }
    return true;
}

void HipRender::setInstanceMotion(bool on)
{
    mInstanceMotion = on;
    if (on)
        return;
    mGuideInstances.clear(), mPrevGuideInstances.clear();
    for (void*& g : mRewound)
    {
        if (mCtx && g)
            skh_buffer_free(mCtx, g);
        g = nullptr;
    }
    if (mCtx)
        check(skh_set_instance_motion(mCtx, nullptr, 0), "skh_set_instance_motion"); // (the library's table goes too)
}

bool HipRender::setHistoryRectification(bool on, const HipRectify* params)
{
    const HipRectify r = params ? *params : HipRectify();
    // (checked here with an image that passes: the real one is render()'s; the fast length through the temporal call it is for)
    float fast = 0.0f;
    const skh_rectify_params probe = hipRectifyParams(r, 1u, 1u, 0.05f, &fast);
    skh_temporal_params fastProbe = hipTemporalParams(HipTemporal(), 1u, 1u, nullptr, 1.0f, 1.0f);
    fastProbe.max_history = fast;
    if (on && (skh_rectify_check(&probe) != SKH_OK || skh_temporal_check(&fastProbe) != SKH_OK))
    {
        mError = "setHistoryRectification: the setting was refused (radius 1 .. 3, k > 0, finite fastHistory >= 1)";
        return false;
    }
    if (!on && !mRectify)
        return true; // (off already: the history stays)
    dropHistory(); // (the two histories start together)
    memset(&mRectifyApplied, 0, sizeof(mRectifyApplied));
    mRectifyFastApplied = 0.0f;
    mRectify = on;
    if (on)
        mRectifySetting = r;
    else
        for (void** g : { &mFast[0], &mFast[1], &mRectifyImage })
        {
            if (mCtx && *g)
                skh_buffer_free(mCtx, *g);
            *g = nullptr;
        }
    return true;
}

bool HipRender::fastHistory(const skh_temporal_params& tp, const void* dColor, const void* normal, const void* position)
{
    if (!mRectify || !mFast[0] || !mFast[1] || !mRectifyImage) // (the three buffers come with the guide buffers: renderGuides)
        return false;
    skh_temporal_params tf = tp;
    hipRectifyParams(mRectifySetting, tp.width, tp.height, tp.albedo_floor, &tf.max_history);
    tf.initial_length = std::min(tf.initial_length, tf.max_history);
    // (without a fast history of its own the stored history is both: read under the shorter max_history it has the length min(n, fastHistory))
    const void* prev = mFastValid ? mFast[mFastStored] : mHistory[mHistoryStored];
    if (!check(skh_temporal(mCtx, &tf, dColor, mGuide[0], normal, position, mGuide[3], prev, mPrevGuide[0], mPrevGuide[1], mPrevGuide[2], mRectifyImage,
                            mFast[1 - mFastStored], nullptr),
               "skh_temporal"))
        return false;
    mRectifyFastApplied = tf.max_history;
    return true; // (the stored fast history stays the stored one until the long history's call has succeeded: rectifyHistory)
}

void HipRender::rectifyHistory(const skh_temporal_params& tp, void* dImage, void* dHistory)
{
    const skh_rectify_params rp = hipRectifyParams(mRectifySetting, tp.width, tp.height, tp.albedo_floor);
    mFastStored = 1 - mFastStored, mFastValid = true; // (the two histories advance together)
    if (check(skh_rectify(mCtx, &rp, dImage, mGuide[0], mGuide[3], dHistory, mFast[mFastStored], dImage, dHistory, nullptr), "skh_rectify"))
        mRectifyApplied = rp;
}

// With object motion on, when the instance tables of the two guide sets differ in a transform: the current set's position and normal planes, rewound into the
// previous frame's world, in mRewound.  false: nothing moved (or the feature is off, or a call failed) -- the caller hands on the true planes.
bool HipRender::rewindGuides(uint32_t width, uint32_t height)
{
    if (!mInstanceMotion || mGuideInstances.empty() || mPrevGuideInstances.empty())
        return false;
    const size_t n = mGuideInstances.size(), nPrev = mPrevGuideInstances.size();
    bool differ = n != nPrev;
    for (size_t i = 0; i < n && !differ; ++i)
        differ = memcmp(mGuideInstances[i].transform, mPrevGuideInstances[i].transform, sizeof(mGuideInstances[i].transform)) != 0;
    if (!differ)
        return false;
    std::vector<skh_instance_motion> table(n);
    for (size_t i = 0; i < n; ++i)
    {
        if (i < nPrev)
            skh_instance_motion_from_transforms(mPrevGuideInstances[i].transform, mGuideInstances[i].transform, &table[i]);
        else
        {
            // an instance the previous frame did not have: no history
            skh_instance_motion_from_transforms(mGuideInstances[i].transform, mGuideInstances[i].transform, &table[i]);
            table[i].flags = SKH_MOTION_MOVED | SKH_MOTION_DROP;
        }
    }
    if (!check(skh_set_instance_motion(mCtx, table.data(), (uint32_t)n), "skh_set_instance_motion"))
        return false;
    for (void*& g : mRewound)
        if (!g && !check(skh_buffer_alloc(mCtx, (size_t)16 * width * height, &g), "skh_buffer_alloc"))
            return false;
    return check(skh_rewind_guides(mCtx, width, height, mGuide[0], mGuide[2], mGuide[1], mRewound[0], mRewound[1]), "skh_rewind_guides");
}

// the four guide planes of the whole image through the pixel centres, into buffers of this object.  With temporal accumulation on, the set rendered last
// (ids, normal, position) and its world_to_clip first become the previous frame's.
bool HipRender::renderGuides()
{
    if (mGuideWidth != mWidth || mGuideHeight != mHeight || (mTemporal && !mHistory[0]) || (mTemporal && mRectify && !mFast[0]))
    {
        freeGuides();
        for (void*& g : mGuide)
            if (!check(skh_buffer_alloc(mCtx, (size_t)16 * mWidth * mHeight, &g), "skh_buffer_alloc"))
                return false;
        if (mTemporal)
            for (void** g : { &mPrevGuide[0], &mPrevGuide[1], &mPrevGuide[2], &mHistory[0], &mHistory[1] })
                if (!check(skh_buffer_alloc(mCtx, (size_t)16 * mWidth * mHeight, g), "skh_buffer_alloc"))
                    return false;
        if (mTemporal && mRectify) // (history rectification's three buffers: here, before the guide pass and the sample, not between two image passes)
            for (void** g : { &mFast[0], &mFast[1], &mRectifyImage })
                if (!check(skh_buffer_alloc(mCtx, (size_t)16 * mWidth * mHeight, g), "skh_buffer_alloc"))
                    return false;
        mGuideWidth = mWidth, mGuideHeight = mHeight;
    }
    skh_aov_params ap;
    if (!aovParams(ap, nullptr, false))
        return false;
    if (mTemporal)
    {
        for (int k = 0; k < 3; ++k)
            std::swap(mGuide[k], mPrevGuide[k]);
        memcpy(mPrevWorldToClip, mGuideWorldToClip, sizeof(mPrevWorldToClip));
        mPrevGuidesValid = mGuidesValid;
        memcpy(mGuideWorldToClip, ap.world_to_clip, sizeof(mGuideWorldToClip));
        if (mInstanceMotion)
        {
            std::swap(mGuideInstances, mPrevGuideInstances);
            mGuideInstances = mSentInstances;
        }
    }
    void* d[SKH_AOV_COUNT] = {};
    d[SKH_AOV_IDS] = mGuide[0], d[SKH_AOV_NORMAL] = mGuide[1], d[SKH_AOV_POSITION] = mGuide[2], d[SKH_AOV_ALBEDO] = mGuide[3];
    const uint32_t planes = (1u << SKH_AOV_IDS) | (1u << SKH_AOV_NORMAL) | (1u << SKH_AOV_POSITION) | (1u << SKH_AOV_ALBEDO);
    mGuidesValid = check(skh_render_aovs(mCtx, &ap, planes, d), "skh_render_aovs");
    return mGuidesValid;
}

void HipRender::uploadMaterials()
{
    Scene& sc = *mScene;
    std::vector<skh_material> mats;
    std::vector<float> emission; // 3 per material: skh_set_emission, after the materials
    std::vector<skh_material_textures> mtex; // one per material: skh_set_material_textures, after the materials
    std::vector<skh_material_cutout> cutouts; // one per material: skh_set_material_cutouts, after the materials
    std::vector<skh_material_blend> blends; // one per material, with setAlphaBlend(true) only: skh_set_material_blend, after the materials
#ifdef SKH_WITH_STRELKA_HEADERS
    // every eTexture parameter becomes one RGBA8 texture (OptixRender.cpp:1346-1377: resolved against resource/searchPath, stbi_load
    // with STBI_rgb_alpha); a file that cannot be read is reported and the material keeps its constant colour (:1195-1199)
    std::vector<std::vector<uint8_t>> pixels;
    std::vector<skh_texture> tex;
    const std::filesystem::path searchPath = getSharedContext().mSettingsManager->getAs<std::string>("resource/searchPath");
    auto load = [&](const std::string& rel) -> uint32_t {
        if (rel.empty())
            return 0u;
        int w = 0, h = 0, ch = 0;
        stbi_uc* data = stbi_load((searchPath / rel).string().c_str(), &w, &h, &ch, STBI_rgb_alpha);
        if (!data)
        {
            std::cerr << "[HipRender] unable to load texture from file: " << rel << std::endl;
            return 0u;
        }
        pixels.emplace_back(data, data + (size_t)w * h * 4);
        stbi_image_free(data);
        tex.push_back(skh_texture{ nullptr, (uint32_t)w, (uint32_t)h });
        return (uint32_t)tex.size(); // 1-based, 0 = none (MDL's resource numbering: texture_support_cuda.h:300-304)
    };
    for (const Scene::MaterialDescription& d : sc.getMaterials())
    {
        const uint32_t diffuseId = load(skhmat::texturePath(d, "diffuse_texture")), normalId = load(skhmat::texturePath(d, "normalmap_texture"));
        mats.push_back(skhmat::translate(d, diffuseId, normalId, mAlphaBlend));
        float le[3];
        skhmat::emission(d, le);
        emission.insert(emission.end(), le, le + 3);
        // roughness / metallic / ORM / emissive maps: loaded through the same path as diffuse_texture
        mtex.push_back(skhmat::materialTextures(d, load));
        // cutout opacity (OmniPBR enable_opacity / opacity_threshold, UsdPreviewSurface opacityThreshold): its map likewise
        cutouts.push_back(skhmat::materialCutout(d, load));
        // fractional opacity (an opacity without a threshold), behind the switch: its map likewise; a blended material does not emit
        if (mAlphaBlend)
        {
            blends.push_back(skhmat::materialBlend(d, load));
            if (blends.back().active)
                std::fill(emission.end() - 3, emission.end(), 0.0f);
        }
    }
    for (size_t k = 0; k < tex.size(); ++k)
        tex[k].rgba8 = pixels[k].data();
#else
    std::vector<skh_texture> tex; // OptixRender.cpp:1352-1377: one texture object per eTexture parameter
    for (const Scene::Texture& t : sc.getTextures())
        tex.push_back(skh_texture{ t.rgba8.data(), t.width, t.height });
    for (const auto& m : sc.getMaterials())
        mats.push_back(m.args);
#endif
    check(skh_set_textures(mCtx, tex.data(), (uint32_t)tex.size()), "skh_set_textures");
    if (mats.empty())
    {
        skh_material m; // default.mdl::default_material registered by init() in the reference (OptixRender.cpp:1090-1097)
        memset(&m, 0, sizeof(m));
        m.base_color[0] = m.base_color[1] = m.base_color[2] = 0.8f;
        mats.push_back(m);
    }
    check(skh_set_materials(mCtx, mats.data(), (uint32_t)mats.size()), "skh_set_materials");
    // emissive meshes: a lamp shade, a screen (all zeros = none: the context then runs the kernels it always ran)
    const bool emits = std::any_of(emission.begin(), emission.end(), [](float v) { return v > 0.0f; });
    check(skh_set_emission(mCtx, emits ? emission.data() : nullptr, emits ? (uint32_t)(emission.size() / 3) : 0u), "skh_set_emission");
    // material textures (no entry binds one = none: likewise)
    const bool maps = std::any_of(mtex.begin(), mtex.end(), [](const skh_material_textures& e) { return e.roughness_texture || e.metallic_texture || e.emission_texture; });
    check(skh_set_material_textures(mCtx, maps ? mtex.data() : nullptr, maps ? (uint32_t)mtex.size() : 0u), "skh_set_material_textures");
    // cutouts (no entry is active = none: likewise)
    const bool cut = std::any_of(cutouts.begin(), cutouts.end(), [](const skh_material_cutout& e) { return e.threshold > 0.0f; });
    check(skh_set_material_cutouts(mCtx, cut ? cutouts.data() : nullptr, cut ? (uint32_t)cutouts.size() : 0u), "skh_set_material_cutouts");
    // fractional opacity (the switch is off, or no entry is active = none: likewise)
    const bool blend = std::any_of(blends.begin(), blends.end(), [](const skh_material_blend& e) { return e.active != 0u; });
    check(skh_set_material_blend(mCtx, blend ? blends.data() : nullptr, blend ? (uint32_t)blends.size() : 0u), "skh_set_material_blend");
}

static void environmentRotation(const float* worldToEnv, float out[9])
{
    static const float identity[9] = { 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f };
    memcpy(out, worldToEnv ? worldToEnv : identity, sizeof(identity));
}

bool HipRender::setEnvironment(const float* rgb, uint32_t width, uint32_t height, const float scale[3], const float* worldToEnv)
{
    skh_environment e;
    e.rgb = rgb;
    e.width = width, e.height = height;
    memcpy(e.scale, scale, sizeof(e.scale));
    environmentRotation(worldToEnv, e.world_to_env);
    mEnvironmentChanged = true;
    return check(skh_set_environment(mCtx, &e), "skh_set_environment");
}

bool HipRender::setEnvironmentTransform(const float scale[3], const float* worldToEnv)
{
    float m[9];
    environmentRotation(worldToEnv, m);
    mEnvironmentChanged = true;
    return check(skh_set_environment_transform(mCtx, scale, m), "skh_set_environment_transform");
}

bool HipRender::applyLightShapes()
{
    return check(skh_set_light_shapes(mCtx, mLightShapes.empty() ? nullptr : mLightShapes.data(), (uint32_t)mLightShapes.size()), "skh_set_light_shapes");
}

bool HipRender::setLightShapes(const skh_light_shape* entries, uint32_t n)
{
    if (entries && n)
        mLightShapes.assign(entries, entries + n);
    else
        mLightShapes.clear();
    mLightShapesChanged = true;
    return mLightsUploaded ? applyLightShapes() : true; // (before the first upload the library has no light list to hold the table against: uploadScene applies it)
}

// the LDR luminance the accumulator's tonemap gives a grey pixel of radiance `radiance` under `exposure`
static float adaptiveDarkLevel(float radiance, const float exposure[3])
{
    float t[3];
    for (int i = 0; i < 3; ++i)
    {
        const float c = radiance * exposure[i];
        t[i] = c / (c + 1.0f);
    }
    return 0.2126f * t[0] + 0.7152f * t[1] + 0.0722f * t[2];
}

bool HipRender::setAdaptiveSampling(float threshold, float darkRadiance, uint32_t minSamples, uint32_t interval)
{
    mConverged = false;
    if (threshold < 0.0f)
    {
        mAdaptive = false;
        return check(skh_set_adaptive(mCtx, nullptr), "skh_set_adaptive");
    }
    skh_adaptive a;
    memset(&a, 0, sizeof(a));
    a.threshold = threshold, a.min_samples = minSamples, a.interval = interval;
    a.dark_level = 1.0f; // (checked here with a level that passes; the real one depends on the exposure: render())
    if (!(darkRadiance > 0.0f) || !std::isfinite(darkRadiance) || skh_adaptive_check(&a) != SKH_OK)
        return false; // (refused; the previous setting stays)
    mAdaptive = true;
    mAdaptiveSetting = a;
    mAdaptiveDarkRadiance = darkRadiance;
    memset(&mAdaptiveApplied, 0, sizeof(mAdaptiveApplied)); // (applied at the next render())
    return true;
}

// ---- first-hit AOVs: skh_render_aovs ----
// inverse of a row-major 4 x 4 in double: Gauss-Jordan with partial pivoting; false: singular
static bool invert4(const double* m, double* out)
{
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 8; ++c)
            a[r][c] = c < 4 ? m[4 * r + c] : (c - 4 == r ? 1.0 : 0.0);
    for (int col = 0; col < 4; ++col)
    {
        int piv = col;
        for (int r = col + 1; r < 4; ++r)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col]))
                piv = r;
        if (a[piv][col] == 0.0)
            return false;
        for (int c = 0; c < 8; ++c)
            std::swap(a[col][c], a[piv][c]);
        const double inv = 1.0 / a[col][col];
        for (int c = 0; c < 8; ++c)
            a[col][c] *= inv;
        for (int r = 0; r < 4; ++r)
        {
            if (r == col)
                continue;
            const double f = a[r][col];
            for (int c = 0; c < 8; ++c)
                a[r][c] -= f * a[col][c];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            out[4 * r + c] = a[r][c + 4];
    return true;
}

bool HipRender::aovParams(skh_aov_params& p, const uint32_t* region, bool sampleZero)
{
    if (!mCtx || !mScene || mWidth == 0 || mHeight == 0)
    {
        mError = "renderAovs: call render() first (the scene and the image size are its)";
        return false;
    }
    memset(&p, 0, sizeof(p));
    Camera& camera = mScene->getCamera(0);
    camera.updateAspectRatio(mWidth / (float)mHeight);
    camera.updateViewMatrix();
    const Mat4 v2w = inverse(camera.matrices.view); // (as render())
    double dv[16], dc[16], iv[16], ic[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
        {
            p.view_to_world[4 * r + c] = v2w[c][r];
            p.clip_to_view[4 * r + c] = camera.matrices.invPerspective[c][r];
            dv[4 * r + c] = p.view_to_world[4 * r + c], dc[4 * r + c] = p.clip_to_view[4 * r + c];
        }
    if (!invert4(dv, iv) || !invert4(dc, ic))
    {
        mError = "renderAovs: the camera's matrices are singular";
        return false;
    }
    // world_to_clip = inverse(clip_to_view) . inverse(view_to_world), in double, rounded once
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
        {
            double s = 0.0;
            for (int k = 0; k < 4; ++k)
                s += ic[4 * r + k] * iv[4 * k + c];
            p.world_to_clip[4 * r + c] = (float)s;
        }
    if (region)
        p.x0 = region[0], p.y0 = region[1], p.width = region[2], p.height = region[3];
    p.sample_index = sampleZero ? 0u : SKH_AOV_PIXEL_CENTRE;
    p.spp_total = getSharedContext().mSettingsManager->getAs<uint32_t>("render/pt/sppTotal");
    p.tmin = getSharedContext().mSettingsManager->getAs<float>("render/pt/dev/materialRayTmin");
    return true;
}

bool HipRender::renderAovs(uint32_t planes, Buffer* const* out, const uint32_t* region, bool sampleZero)
{
    skh_aov_params p;
    if (!aovParams(p, region, sampleZero))
        return false;
    const uint64_t pixels = region ? (uint64_t)region[2] * region[3] : (uint64_t)mWidth * mHeight;
    void* d[SKH_AOV_COUNT] = {};
    for (uint32_t k = 0; k < SKH_AOV_COUNT; ++k)
    {
        if (!((planes >> k) & 1u))
            continue;
        if (!out || !out[k] || out[k]->getFormat() != BufferFormat::FLOAT4 || (uint64_t)out[k]->width() * out[k]->height() < pixels)
        {
            mError = "renderAovs: plane " + std::to_string(k) + " needs a FLOAT4 buffer of the region's size";
            return false;
        }
        d[k] = static_cast<HipBuffer*>(out[k])->getNativePtr();
    }
    // (a refusal is the caller's arguments, not a broken renderer: reported, not asserted)
    if (skh_render_aovs(mCtx, &p, planes, d) != SKH_OK)
    {
        mError = std::string("skh_render_aovs: ") + skh_last_error(mCtx);
        return false;
    }
    return true;
}

bool HipRender::pick(uint32_t x, uint32_t y, HipPick& out)
{
    const uint32_t region[4] = { x, y, 1u, 1u };
    skh_aov_params p;
    if (!aovParams(p, region, false))
        return false;
    void* d = nullptr; // the seven planes of one pixel, back to back
    if (skh_buffer_alloc(mCtx, 16 * SKH_AOV_COUNT, &d) != SKH_OK)
    {
        mError = std::string("skh_buffer_alloc: ") + skh_last_error(mCtx);
        return false;
    }
    void* planes[SKH_AOV_COUNT];
    for (uint32_t k = 0; k < SKH_AOV_COUNT; ++k)
        planes[k] = static_cast<char*>(d) + 16 * k;
    uint32_t w[4 * SKH_AOV_COUNT];
    const bool ok = skh_render_aovs(mCtx, &p, (1u << SKH_AOV_COUNT) - 1u, planes) == SKH_OK && skh_buffer_download(mCtx, d, w, sizeof(w)) == SKH_OK;
    if (!ok)
        mError = std::string("pick: ") + skh_last_error(mCtx);
    skh_buffer_free(mCtx, d);
    if (!ok)
        return false;
    float f[4 * SKH_AOV_COUNT];
    memcpy(f, w, sizeof(f));
    out.instanceId = w[0], out.primId = w[1], out.material = w[2], out.kind = w[3];
    out.t = f[4 * SKH_AOV_HIT], out.u = f[4 * SKH_AOV_HIT + 1], out.v = f[4 * SKH_AOV_HIT + 2], out.depth = f[4 * SKH_AOV_HIT + 3];
    for (int k = 0; k < 3; ++k)
    {
        out.normal[k] = f[4 * SKH_AOV_NORMAL + k], out.position[k] = f[4 * SKH_AOV_POSITION + k];
        out.geomNormal[k] = f[4 * SKH_AOV_GEOM_NORMAL + k], out.albedo[k] = f[4 * SKH_AOV_ALBEDO + k];
    }
    out.facing = f[4 * SKH_AOV_NORMAL + 3];
    out.texcoord[0] = f[4 * SKH_AOV_TEXCOORD], out.texcoord[1] = f[4 * SKH_AOV_TEXCOORD + 1];
    return true;
}

void HipRender::render(Buffer* output)
{
    SharedContext& sh = getSharedContext();
    if (mLightShapesChanged)
    {
        sh.mSubframeIndex = 0; // other lights: the accumulated image is of the old ones
        mLightShapesChanged = false;
        dropHistory();
    }
    if (mEnvironmentChanged)
    {
        sh.mSubframeIndex = 0; // a new sky: the accumulated image is of the old one
        mEnvironmentChanged = false;
        dropHistory();
    }
    if (sh.mFrameNumber == 0)
        uploadScene(); // scene is uploaded once (OptixRender.cpp:876-888); later edits are ignored, like the reference, except ...
    else if (!mScene->getDirtyInstances().empty() && sendMovedInstances())
        sh.mSubframeIndex = 0; // ... moved instances (Scene::updateInstanceTransform): the hierarchy is updated, accumulation restarts as after a camera move

    const uint32_t width = output->width();
    const uint32_t height = output->height();
    // updatePathtracerParams (OptixRender.cpp:827-872)
    if (mWidth != width || mHeight != height)
    {
        sh.mSubframeIndex = 0;
        sh.mSettingsManager->setAs<bool>("render/pt/isResized", true);
        dropHistory();
        applyTiles(width, height);
        check(skh_resize(mCtx, width, height), "skh_resize");
        mWidth = width;
        mHeight = height;
    }
    Camera& camera = mScene->getCamera(0);
    camera.updateAspectRatio(width / (float)height);
    camera.updateViewMatrix();
    const bool cameraChanged = camera.matrices.perspective != mPrevPerspective || camera.matrices.view != mPrevView;
    if (cameraChanged)
        sh.mSubframeIndex = 0; // need reset (OptixRender.cpp:903-908)

    SettingsManager& settings = *sh.mSettingsManager;
    bool settingsChanged = false;
    const uint32_t rectLightSamplingMethod = settings.getAs<uint32_t>("render/pt/rectLightSamplingMethod");
    settingsChanged = (mRectLightSamplingMethodPrev != rectLightSamplingMethod);
    mRectLightSamplingMethodPrev = rectLightSamplingMethod;
    bool enableAccumulation = settings.getAs<bool>("render/pt/enableAcc");
    settingsChanged |= (mEnableAccumulationPrev != enableAccumulation);
    mEnableAccumulationPrev = enableAccumulation;
    const uint32_t sspTotal = settings.getAs<uint32_t>("render/pt/sppTotal");
    settingsChanged |= (mSppTotalPrev > sspTotal); // reset only if the new spp is below what was already accumulated
    mSppTotalPrev = sspTotal;
    const float gamma = settings.getAs<float>("render/post/gamma");
    const uint32_t tonemapperType = settings.getAs<uint32_t>("render/pt/tonemapperType");
    if (settingsChanged)
    {
        sh.mSubframeIndex = 0;
        dropHistory();
    }

    skh_frame_params p;
    memset(&p, 0, sizeof(p));
    p.max_depth = settings.getAs<uint32_t>("render/pt/depth");
    p.rect_light_sampling_method = rectLightSamplingMethod;
    p.debug = settings.getAs<uint32_t>("render/pt/debug");
    p.shadow_ray_tmin = settings.getAs<float>("render/pt/dev/shadowRayTmin");
    p.material_ray_tmin = settings.getAs<float>("render/pt/dev/materialRayTmin");
    // glm::transpose(glm::inverse(view)) / glm::transpose(invPerspective) memcpy'd column-major == row-major matrices
    const Mat4 v2w = inverse(camera.matrices.view); // (glm::inverse / oka::inverse, found by ADL)
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
        {
            p.view_to_world[4 * r + c] = v2w[c][r];
            p.clip_to_view[4 * r + c] = camera.matrices.invPerspective[c][r];
        }
    p.subframe_index = (uint32_t)sh.mSubframeIndex;
    // photometric exposure (OptixRender.cpp:961-987)
    const float filmIso = settings.getAs<float>("render/post/tonemapper/filmIso");
    const float cm2_factor = settings.getAs<float>("render/post/tonemapper/cm2_factor");
    const float fStop = settings.getAs<float>("render/post/tonemapper/fStop");
    const float shutterSpeed = settings.getAs<float>("render/post/tonemapper/shutterSpeed");
    float e[3] = { 1.0f, 1.0f, 1.0f };
    const float lum = e[0] * 0.299f + e[1] * 0.587f + e[2] * 0.114f;
    const float k = filmIso > 0.0f ? cm2_factor * filmIso / (shutterSpeed * fStop * fStop) / 100.0f : cm2_factor;
    const float invLum = 1.0f / lum;
    for (int i = 0; i < 3; ++i)
        p.exposure[i] = e[i] * k * invLum;

    const uint32_t totalSpp = sspTotal;
    const uint32_t samplesPerLaunch = settings.getAs<uint32_t>("render/pt/spp");
    const int32_t leftSpp = (int32_t)totalSpp - (int32_t)sh.mSubframeIndex;
    uint32_t samplesThisLaunch = enableAccumulation ? (uint32_t)std::min((int32_t)samplesPerLaunch, leftSpp) : samplesPerLaunch;
    if (p.debug == 1)
    {
        samplesThisLaunch = 1;
        enableAccumulation = false;
    }
    // temporal accumulation: a moving camera's frame is one raw sample of the sequence, another one every time (HipRender.h, rotateSamples)
    const bool temporalFrame = mTemporal && p.debug == 0 && (!mSharing || mRank == 0);
    const bool startCall = sh.mSubframeIndex == 0;
    if (mTemporal && mTemporalSetting.rotateSamples && !mSharing && p.debug == 0 && enableAccumulation && startCall && cameraChanged && mRendered && totalSpp != 0u)
    {
        p.subframe_index = mRotation++ % totalSpp;
        samplesThisLaunch = std::min(samplesPerLaunch, totalSpp - p.subframe_index);
        enableAccumulation = false; // (below: mSubframeIndex stays 0, the first still call starts a normal accumulation at sample 0)
    }
    p.samples_this_launch = samplesThisLaunch;
    p.enable_accumulation = enableAccumulation;
    p.spp_total = totalSpp;
    mLastSubframeIndex = p.subframe_index, mLastEnableAccumulation = p.enable_accumulation;

    void* dImage = static_cast<HipBuffer*>(output)->getNativePtr();
    const bool adaptiveFrame = mAdaptive && enableAccumulation && p.debug == 0;
    if (mAdaptive)
    {
        // the setting under this frame's exposure; a changed one restarts the library's adaptive frame (all tiles active)
        skh_adaptive a = mAdaptiveSetting;
        a.dark_level = adaptiveDarkLevel(mAdaptiveDarkRadiance, p.exposure);
        if (memcmp(&a, &mAdaptiveApplied, sizeof(a)) != 0 && check(skh_set_adaptive(mCtx, &a), "skh_set_adaptive"))
            mAdaptiveApplied = a;
    }
    if (sh.mSubframeIndex == 0 || !adaptiveFrame)
        mConverged = false;
    // the denoiser's guide planes belong to the accumulation: rendered when it (re)starts or the image size changed, before the frame's own work
    const bool denoiseFrame = mDenoise && p.debug == 0 && (!mSharing || mRank == 0);
    if ((denoiseFrame || temporalFrame) && (startCall || !mGuidesValid || mGuideWidth != width || mGuideHeight != height))
        renderGuides();
    if (samplesThisLaunch != 0 && !mConverged)
    {
        check(skh_render_subframe(mCtx, &p, dImage), "skh_render_subframe");
        if (enableAccumulation)
            sh.mSubframeIndex += samplesThisLaunch;
        else
            sh.mSubframeIndex = 0;
        skh_adaptive_info info;
        if (adaptiveFrame && check(skh_get_adaptive_info(mCtx, &info), "skh_get_adaptive_info"))
            mConverged = info.enabled != 0u && info.checks != 0u && info.active_tiles == 0u; // no active tile left: as sppTotal reached, from the next render() on
    }
    else
    {
        // all spp done: the latest accumulated RAW radiance -- or, for the debug views 2 / 3, the raw diffuse / specular AOV -- goes back
        // to the image before every tonemap() below (OptixRender.cpp:1022-1043); without the copy the in-place tonemap would be applied to
        // an already tonemapped image call after call
        if (p.debug == 0)
            check(skh_copy_accum(mCtx, dImage), "skh_copy_accum");
        else if (p.debug == 2 || p.debug == 3)
            check(skh_copy_aov(mCtx, p.debug - 2, dImage), "skh_copy_aov");
    }
    if (mSharing && p.debug == 0 && enableAccumulation)
    {
        // the frame's one collective: every rank's tile accumulators -> rank 0, whose output then holds the whole image
        check(skh_gather_tiles(mCtx, mMaxTiles, mRank == 0 ? mGatherBuf : nullptr, 0), "skh_gather_tiles");
        if (mRank == 0)
            check(skh_scatter_tiles(mCtx, mGatherBuf, mAllTileXY.data(), (uint32_t)(mAllTileXY.size() / 2), mTileSize, dImage, width, height),
                  "skh_scatter_tiles");
    }
    // variance guidance replaces this call's skh_temporal + skh_denoise pair by skh_temporal + skh_moments + skh_denoise_variance: only with both features on, only
    // on a call that starts an accumulation, and only once its four buffers exist
    bool guided = mVariance && temporalFrame && denoiseFrame && mGuidesValid && startCall;
    if (guided && !mVarianceImage)
        for (void** g : { &mVarianceImage, &mMotion, &mMoments[0], &mMoments[1] })
            guided = guided && check(skh_buffer_alloc(mCtx, (size_t)16 * width * height, g), "skh_buffer_alloc");
    if (guided)
    {
        const int next = 1 - mHistoryStored, nextMoments = 1 - mMomentsStored;
        const bool had = mHistoryValid && mPrevGuidesValid, hadMoments = had && mMomentsValid;
        const skh_temporal_params tp = hipTemporalParams(mTemporalSetting, width, height, had ? mPrevWorldToClip : nullptr, 1.0f, mSceneDiagonal);
        const skh_vdenoise_params vp = hipVarianceParams(mVarianceSetting, mDenoiseSetting, width, height, p.exposure, mSceneDiagonal);
        // moved instances: the reprojection's normal and position are the rewound planes; the filter keeps the true ones
        const bool rewound = had && rewindGuides(width, height);
        const void* tNormal = rewound ? mRewound[1] : mGuide[1];
        const void* tPosition = rewound ? mRewound[0] : mGuide[2];
        // history rectification: the fast history first, from the same planes
        const bool rectified = had && fastHistory(tp, dImage, tNormal, tPosition);
        // the blended image goes to this object's buffer: the output image keeps the raw sample for skh_moments, then takes the filtered result
        if (check(skh_temporal(mCtx, &tp, dImage, mGuide[0], tNormal, tPosition, mGuide[3], had ? mHistory[mHistoryStored] : nullptr, mPrevGuide[0], mPrevGuide[1],
                               mPrevGuide[2], mVarianceImage, mHistory[next], mMotion),
                  "skh_temporal"))
        {
            mFastValid = false; // (the history stored here is both, unless the next line stores a fast one beside it)
            if (rectified)
                rectifyHistory(tp, mVarianceImage, mHistory[next]);
            mHistoryStored = next, mHistoryValid = true;
            mTemporalApplied = tp, mTemporalHadPrevious = had;
            if (check(skh_moments(mCtx, &tp, dImage, mGuide[0], tPosition, mGuide[3], hadMoments ? mMotion : nullptr, hadMoments ? mMoments[mMomentsStored] : nullptr,
                                  mMoments[nextMoments]),
                      "skh_moments"))
            {
                mMomentsStored = nextMoments, mMomentsValid = true;
                mMomentsHadPrevious = hadMoments;
                if (check(skh_denoise_variance(mCtx, &vp, mVarianceImage, mGuide[0], mGuide[1], mGuide[2], mGuide[3], mMoments[mMomentsStored], dImage, nullptr),
                          "skh_denoise_variance"))
                    mVarianceApplied = vp;
            }
            else
                mMomentsValid = false;
        }
    }
    if (!guided && temporalFrame && mGuidesValid)
    {
        // the output image -- linear here --; the accumulator is not touched
        const int next = 1 - mHistoryStored;
        if (startCall)
        {
            // the stored history, reprojected into the new frame and blended with it, in place; the new history takes the stored one's place
            const bool had = mHistoryValid && mPrevGuidesValid;
            const skh_temporal_params tp = hipTemporalParams(mTemporalSetting, width, height, had ? mPrevWorldToClip : nullptr, 1.0f, mSceneDiagonal);
            const bool rewound = had && rewindGuides(width, height); // (moved instances: the rewound normal and position planes)
            const void* tNormal = rewound ? mRewound[1] : mGuide[1];
            const void* tPosition = rewound ? mRewound[0] : mGuide[2];
            // history rectification: the fast history first, while the output image still holds the raw sample
            const bool rectified = had && fastHistory(tp, dImage, tNormal, tPosition);
            if (check(skh_temporal(mCtx, &tp, dImage, mGuide[0], tNormal, tPosition, mGuide[3], had ? mHistory[mHistoryStored] : nullptr, mPrevGuide[0], mPrevGuide[1],
                                   mPrevGuide[2], dImage, mHistory[next], nullptr),
                      "skh_temporal"))
            {
                mFastValid = false; // (the history stored here is both, unless the next line stores a fast one beside it)
                if (rectified)
                    rectifyHistory(tp, dImage, mHistory[next]);
                mHistoryStored = next, mHistoryValid = true;
                mTemporalApplied = tp, mTemporalHadPrevious = had;
            }
        }
        else
        {
            // an accumulation in progress: its image is shown as it is, and becomes the history with its true length (the call's image output goes to the
            // history buffer that is not the stored one, and is discarded)
            skh_temporal_params tp = hipTemporalParams(mTemporalSetting, width, height, nullptr, 1.0f, mSceneDiagonal);
            tp.initial_length = std::min((float)sh.mSubframeIndex, tp.max_history); // (the samples in the accumulator: >= 1 here)
            if (check(skh_temporal(mCtx, &tp, dImage, mGuide[0], mGuide[1], mGuide[2], mGuide[3], nullptr, nullptr, nullptr, nullptr, mHistory[next],
                                   mHistory[mHistoryStored], nullptr),
                      "skh_temporal"))
            {
                mHistoryValid = true, mFastValid = false; // (the accumulator is both histories)
                mTemporalApplied = tp, mTemporalHadPrevious = false;
            }
        }
    }
    if (!guided && denoiseFrame && mGuidesValid)
    {
        // the output image -- linear here --, in place; the accumulator is not touched
        const skh_denoise_params dn = hipDenoiseParams(mDenoiseSetting, width, height, p.exposure, mSceneDiagonal);
        if (check(skh_denoise(mCtx, &dn, dImage, mGuide[0], mGuide[1], mGuide[2], mGuide[3], dImage), "skh_denoise"))
            mDenoiseApplied = dn;
    }
    if (p.debug != 1)
        check(skh_tonemap(mCtx, dImage, width, height, tonemapperType, p.exposure, gamma), "skh_tonemap");
    output->unmap();
    sh.mFrameNumber++;
    mPrevView = camera.matrices.view;
    mPrevPerspective = camera.matrices.perspective;
    mRendered = true;
}

#ifndef SKH_WITH_STRELKA_HEADERS
// (in the Strelka tree RenderFactory lives in src/render/render.cpp: integration/strelka_hip.patch adds the eCompute branch there)
Render* RenderFactory::createRender(RenderType type)
{
    if (type == RenderType::eCompute)
        return new HipRender();
    return nullptr; // eOptiX / eMetal live in the reference tree
}
Render* RenderFactory::createRender()
{
    return new HipRender();
}
#endif

} // namespace oka
