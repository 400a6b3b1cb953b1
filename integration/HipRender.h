// oka::HipRender -- the MI355X backend behind Strelka's render interface, in the RenderType::eCompute slot the reference declares but
// never implements (include/render/render.h:9-14, src/render/render.cpp:10-26).  What OptiXRender / OptixBuffer are to OptiX
// (src/render/optix/OptixRender.{h,cpp}, OptixBuffer.{h,cpp}), these two classes are to libstrelka_hip.so (include/strelka_hip.h).
//
// ONE source, two sets of headers (a host-side include switch only -- the device code has a single path):
//   -DSKH_WITH_STRELKA_HEADERS   inside the Strelka tree: <render/render.h>, <render/buffer.h>, <scene/scene.h>, <settings/settings.h>
//                                 (glm types; integration/strelka_hip.cmake + strelka_hip.patch wire it in)
//   otherwise                     strelka_amd/host/oka_mirror.h, this repository's dependency-free stand-in for those headers
//                                 (what the tests and the benchmark box compile: glm / MDL SDK / OpenUSD are not in this image)
// The code below uses only what both provide: m[col][row] element access, inverse(m) found by ADL, operator!= on matrices, the
// scene's flat-array getters, SettingsManager::getAs / setAs.
#pragma once
#ifdef SKH_WITH_STRELKA_HEADERS
#    include <render/render.h>
#    include <render/buffer.h>
#    include <scene/scene.h>
#    include <settings/settings.h>
#    include <strelka_hip.h>
#else
#    include "../strelka_amd/host/oka_mirror.h"
#endif

#include <cmath>
#include <string>
#include <vector>

namespace oka
{

class HipBuffer : public Buffer // OptixBuffer.{h,cpp}
{
public:
    HipBuffer(skh_context* ctx, void* devicePtr, BufferFormat format, uint32_t width, uint32_t height);
    ~HipBuffer() override;
    void resize(uint32_t width, uint32_t height) override;
    void* map() override; // D2H into mHostData, returns nullptr like OptixBuffer::map (OptixBuffer.cpp:37-43)
    void unmap() override
    {
    }
    void* getNativePtr()
    {
        return mDeviceData;
    }

private:
    skh_context* mCtx;
    void* mDeviceData = nullptr;
    void* mRegistered = nullptr; // mHostData's storage while it is page-locked (skh_host_register)
};

struct HipPick // HipRender::pick: the words of skh_render_aovs' seven planes at one pixel
{
    uint32_t instanceId, primId, material, kind; // kind: 0 miss, 1 triangle, 2 curve segment, 3 light proxy; the ids are 0xffffffff at a miss
    float t, u, v, depth;
    float normal[3], facing;
    float position[3];
    float geomNormal[3];
    float albedo[3];
    float texcoord[2];
};

struct HipDenoise // HipRender::setDenoiser: a field that is 0 (or negative) takes its default
{
    uint32_t levels = 0;        // 5
    float sigmaColor = 0.0f;    // radiance; default: 1 / the mean of the frame's three exposure factors -- what a Reinhard tonemap under that exposure shows as mid-grey
    float sigmaNormal = 0.0f;   // 0.3
    float sigmaPlane = 0.0f;    // scene units; default: planeFraction x the diagonal of the scene's bounding box
    float planeFraction = 0.0f; // 0.005
    float albedoFloor = 0.0f;   // 0.05
};

// the skh_denoise_params render() hands to skh_denoise for a HipDenoise setting: levels 0 .. levels - 1, both flags (the image is demodulated before the first
// level and remodulated after the last)
inline skh_denoise_params hipDenoiseParams(const HipDenoise& d, uint32_t width, uint32_t height, const float exposure[3], float sceneDiagonal)
{
    skh_denoise_params p = {};
    p.width = width, p.height = height;
    p.first_level = 0u, p.levels = d.levels ? d.levels : 5u;
    const float meanExposure = (exposure[0] + exposure[1] + exposure[2]) / 3.0f;
    p.sigma_color = d.sigmaColor > 0.0f ? d.sigmaColor : 1.0f / meanExposure;
    p.sigma_normal = d.sigmaNormal > 0.0f ? d.sigmaNormal : 0.3f;
    const float plane = d.sigmaPlane > 0.0f ? d.sigmaPlane : (d.planeFraction > 0.0f ? d.planeFraction : 0.005f) * sceneDiagonal;
    p.sigma_plane = plane > 0.0f ? plane : HUGE_VALF; // (no mesh instance to measure: the term is off)
    p.albedo_floor = d.albedoFloor > 0.0f ? d.albedoFloor : 0.05f;
    p.flags = SKH_DENOISE_DEMODULATE | SKH_DENOISE_REMODULATE;
    return p;
}

struct HipTemporal // HipRender::setTemporal: a field that is 0 takes its default
{
    float normalMin = 0.0f;      // 0.9; another value is taken as it is (-1 turns the test off)
    float planeTolerance = 0.0f; // scene units; default (also for a negative value): planeFraction x the diagonal of the scene's bounding box
    float planeFraction = 0.0f;  // 0.005, the denoiser's fraction
    float maxHistory = 0.0f;     // 32
    float albedoFloor = 0.0f;    // 0.05
    bool rotateSamples = true;   // a moving camera's frames take successive samples of the sequence instead of sample 0 every time
};

// the skh_temporal_params render() hands to skh_temporal for a HipTemporal setting: DEMODULATE; prevWorldToClip nullptr = no previous frame (the identity, which
// the check accepts); initialLength 0 = 1
inline skh_temporal_params hipTemporalParams(const HipTemporal& t, uint32_t width, uint32_t height, const float* prevWorldToClip, float initialLength, float sceneDiagonal)
{
    skh_temporal_params p = {};
    p.width = width, p.height = height;
    for (int k = 0; k < 16; ++k)
        p.prev_world_to_clip[k] = prevWorldToClip ? prevWorldToClip[k] : (k % 5 == 0 ? 1.0f : 0.0f);
    p.normal_min = t.normalMin != 0.0f ? t.normalMin : 0.9f;
    const float plane = t.planeTolerance > 0.0f ? t.planeTolerance : (t.planeFraction > 0.0f ? t.planeFraction : 0.005f) * sceneDiagonal;
    p.plane_tolerance = plane > 0.0f ? plane : HUGE_VALF; // (no mesh instance to measure: the test is off)
    p.max_history = t.maxHistory > 0.0f ? t.maxHistory : 32.0f;
    p.initial_length = initialLength > 0.0f ? initialLength : 1.0f;
    p.albedo_floor = t.albedoFloor > 0.0f ? t.albedoFloor : 0.05f;
    p.flags = SKH_TEMPORAL_DEMODULATE;
    return p;
}

struct HipVariance // HipRender::setVarianceGuidance: a field that is 0 (or negative) takes its default
{
    float sigmaLuminance = 0.0f; // 0.25: the luminance term is 1 at a quarter of the local per-sample standard deviation (docs/LOG.md has the table)
    float epsilon = 0.0f;        // luminance; default: 0.01 / the mean of the frame's three exposure factors -- a hundredth of HipDenoise's default sigmaColor
    float minHistory = 0.0f;     // 4: moments younger than this take the spatial estimate
};

// the skh_vdenoise_params render() hands to skh_denoise_variance: the levels, sigmaNormal, sigmaPlane and albedoFloor of the HipDenoise setting (hipDenoiseParams'
// defaults), the three fields of the HipVariance setting, all three flags
inline skh_vdenoise_params hipVarianceParams(const HipVariance& v, const HipDenoise& d, uint32_t width, uint32_t height, const float exposure[3], float sceneDiagonal)
{
    const skh_denoise_params dn = hipDenoiseParams(d, width, height, exposure, sceneDiagonal);
    skh_vdenoise_params p = {};
    p.width = width, p.height = height;
    p.first_level = dn.first_level, p.levels = dn.levels;
    p.sigma_luminance = v.sigmaLuminance > 0.0f ? v.sigmaLuminance : 0.25f;
    p.sigma_normal = dn.sigma_normal, p.sigma_plane = dn.sigma_plane, p.albedo_floor = dn.albedo_floor;
    const float meanExposure = (exposure[0] + exposure[1] + exposure[2]) / 3.0f;
    p.epsilon = v.epsilon > 0.0f ? v.epsilon : 0.01f / meanExposure;
    p.min_history = v.minHistory > 0.0f ? v.minHistory : 4.0f;
    p.flags = SKH_DENOISE_DEMODULATE | SKH_DENOISE_REMODULATE | SKH_VDENOISE_ESTIMATE;
    return p;
}

struct HipRectify // HipRender::setHistoryRectification: a numeric field that is 0 takes its default (docs/LOG.md, "History rectification", has the table they come from)
{
    uint32_t radius = 0;       // 1: a 3 x 3 window; 2 and 3 are legal
    float k = 0.0f;            // 2: the long history is clamped to the fast one's mean +- 2 standard deviations
    float fastHistory = 0.0f;  // 4: the fast history's max_history
    bool shorten = true;       // a clamped pixel's history is no longer than its fast history (SKH_RECTIFY_SHORTEN)
};

// the skh_rectify_params render() hands to skh_rectify for a HipRectify setting: REMODULATE (hipTemporalParams demodulates), the temporal call's albedo floor;
// *fastHistory, when given: the max_history of the fast history's skh_temporal call
inline skh_rectify_params hipRectifyParams(const HipRectify& r, uint32_t width, uint32_t height, float albedoFloor, float* fastHistory = nullptr)
{
    skh_rectify_params p = {};
    p.width = width, p.height = height;
    p.radius = r.radius != 0u ? r.radius : 1u;
    p.k = r.k != 0.0f ? r.k : 2.0f;
    p.albedo_floor = albedoFloor;
    p.flags = SKH_RECTIFY_REMODULATE | (r.shorten ? SKH_RECTIFY_SHORTEN : 0u);
    if (fastHistory)
        *fastHistory = r.fastHistory != 0.0f ? r.fastHistory : 4.0f;
    return p;
}

class HipRender : public Render
{
public:
    using Mat4 = decltype(Camera::Matrices::view); // glm::float4x4 in the Strelka tree, oka::float4x4 in the mirror

    HipRender() = default;
    ~HipRender() override;
    void init() override; // OptiXRender::init (OptixRender.cpp:1059-1105): context + default material 0
    void render(Buffer* output) override; // OptiXRender::render (OptixRender.cpp:874-1057)
    Buffer* createBuffer(const BufferDesc& desc) override; // OptixRender.cpp:1107-1115
    void* getNativeDevicePtr() override
    {
        return mCtx;
    }
    const std::string& lastError() const
    {
        return mError;
    }
    skh_context* context()
    {
        return mCtx;
    }
    // Multi-GPU (new: the reference is one process on one GPU).  One HipRender per process per GPU; this one renders the pixel
    // tiles t = rank (mod worldSize) of every frame -- the split is by tile because the accumulator is an order-dependent LDR-space
    // lerp per pixel (OptixRender.cu:60-78): sharding by samples would change the image -- and after every render() the tile
    // accumulators of all ranks are gathered to rank 0 below the C ABI (skh_gather_tiles: RCCL sends over xGMI), whose output
    // buffer then holds the whole frame (the other ranks' buffers hold their own tiles).  commId: 128 bytes from
    // skh_comm_unique_id on rank 0, handed to every rank by whatever launched the processes.  Call after init(), before render().
    bool enableTileSharing(const void* commId, int worldSize, int rank, uint32_t tileSize = 32);
    // Environment (dome) light (new: the reference lists HdPrimTypeTokens->domeLight and never creates one).  rgb: width x height x 3 linear floats, lat-long,
    // row 0 = the +Y pole, column 0 at phi = 0 on +X, phi towards +Z; nullptr removes it.  scale = intensity x colour; worldToEnv = row-major 3x3 rotation
    // (nullptr = identity).  Accumulation restarts at the next render(), as after a camera move.  With tile sharing every rank makes the same call.
    // Call after init().  INTEGRATION.md says how an HdStrelkaLight of type domeLight feeds it.
    bool setEnvironment(const float* rgb, uint32_t width, uint32_t height, const float scale[3], const float* worldToEnv = nullptr);
    // the same map under a new intensity x colour and rotation: no table rebuild (a viewer spinning its dome)
    bool setEnvironmentTransform(const float scale[3], const float* worldToEnv = nullptr);
    // Light shapes (new: the reference's UniformLightDesc has no shaping fields, and its disk light is never sampled).  One skh_light_shape per light, indexed as
    // Scene::getLights() is: SKH_LIGHT_SHAPE_SAMPLE_DISC lets a disk light take part in next-event estimation, SKH_LIGHT_SHAPE_CONE narrows a rect, disk or
    // sphere light by a UsdLux ShapingAPI cone (include/strelka_hip.h has the definitions).  nullptr / 0 removes the table.  The table is kept: it is applied at
    // once when the scene is uploaded already, and again after every upload of the light list.  Accumulation restarts at the next render().  With tile
    // sharing every rank makes the same call.  INTEGRATION.md says what an HdStrelkaLight hands over.
    bool setLightShapes(const skh_light_shape* entries, uint32_t n);
    // Fractional opacity (skh_set_material_blend), OFF by default: with it, a material description whose opacity has no threshold -- OmniPBR enable_opacity without
    // opacity_threshold, UsdPreviewSurface opacity < 1 without opacityThreshold -- is uploaded as a PBR material with a blend entry (skhmat::materialBlend), not as
    // glass or opaque.  Call before init() / before the materials are uploaded.
    void setAlphaBlend(bool on)
    {
        mAlphaBlend = on;
    }
    // Adaptive sampling (skh_set_adaptive; new: the reference's only stopping rule is sppTotal), OFF by default: what Hydra's convergedVariance and
    // convergedSamplesPerPixel render settings and HdRenderPass::IsConverged ask of a delegate.  A tile stops once the relative standard error of every pixel's
    // tonemapped luminance is at most `threshold`; darkRadiance is the scene radiance below which the error is taken relative to that level (turned into the
    // LDR level under the frame's exposure at every render()); checks after minSamples launches and every `interval` after.  threshold < 0 turns it off.
    // false: a parameter was refused (the previous setting stays).  Call after init().  With tile sharing every rank makes the same call.
    bool setAdaptiveSampling(float threshold, float darkRadiance, uint32_t minSamples, uint32_t interval);
    // true once no tile of this frame is active any more: render() then hands back the accumulated image as it does when sppTotal is reached, until something
    // restarts the accumulation
    bool isConverged() const
    {
        return mConverged;
    }
    // First-hit AOVs (skh_render_aovs; new: the reference renders one image and nothing tells a host what is under a pixel).  planes: bit k = plane SKH_AOV_k;
    // out[k]: a FLOAT4 buffer from createBuffer of at least the region's size for every set bit (the ids plane holds four uint32 per pixel in it), else ignored;
    // region: {x0, y0, width, height} of the last render()'s image, nullptr = all of it; sampleZero: the camera ray of sample 0 of sppTotal (the first hit of the
    // first path render() traces per pixel) instead of the ray through the pixel centre.  The camera is the one render() reads; call after the first render().
    // The frame being accumulated is not disturbed.  false: refused or failed (lastError()).  INTEGRATION.md maps the planes to Hydra's AOVs.
    bool renderAovs(uint32_t planes, Buffer* const* out, const uint32_t* region = nullptr, bool sampleZero = false);
    // what is under pixel (x, y): a 1 x 1 region of every plane, through the pixel centre
    bool pick(uint32_t x, uint32_t y, HipPick& out);
    // the parameters renderAovs hands to skh_render_aovs for the current camera (world_to_clip: the two inverses in double, rounded once)
    bool aovParams(skh_aov_params& p, const uint32_t* region, bool sampleZero);
    // Denoiser (skh_denoise; new: the reference hands back raw samples), OFF by default.  With it on, render() with debug == 0 filters the OUTPUT image -- linear at
    // that point -- between skh_render_subframe and skh_tonemap.  The accumulator is never filtered: the frame converges to what it converged to before.  The guide
    // planes (ids, normal, position, albedo through the pixel centres: renderAovs' parameters) live in buffers this object owns and are rendered again only when
    // the accumulation restarts -- a camera change, a scene change, a settings change -- or the image size changes.  With tile sharing rank 0 filters the gathered
    // image.  params == nullptr: every default.  false: the setting was refused (skh_denoise_check; the previous one stays).  With it off, render() makes the calls
    // it made before.  INTEGRATION.md has the defaults' reasons.
    bool setDenoiser(bool on, const HipDenoise* params = nullptr);
    // what the last filtered render() handed to skh_denoise (false: none yet)
    bool denoiseParams(skh_denoise_params& p) const
    {
        p = mDenoiseApplied;
        return mDenoiseApplied.width != 0u;
    }
    // Temporal accumulation (skh_temporal; new: in the reference every camera move starts from one sample), OFF by default.  With it on, render() with debug == 0
    // ends with exactly one skh_temporal call on the OUTPUT image -- after the gather, before skh_denoise when that is on, before the tonemap; the accumulator is
    // never touched.  This object owns two history buffers and a second set of ids / normal / position guide buffers; the guide pass is the denoiser's
    // renderGuides(), once per accumulation whichever of the two features is on.
    //   a call that starts an accumulation       reprojects the stored history into the new frame, stores the new history, and the guide sets change places
    //   a call that continues one                shows the accumulator's image as before and stores it as the history, with its true length
    //                                            min(samples accumulated, maxHistory): skh_temporal without a previous frame, its image output discarded
    //   the history is dropped after             a resize, setLightShapes / setEnvironment changes, the settings changes that restart the accumulation, setTemporal.
    //                                            Moved instances keep it: the plane test answers for the geometry, and their shadows on other surfaces
    //                                            follow within a few frames with setHistoryRectification
    //   rotateSamples                            a start call whose camera differs from the previous call's is traced with enable_accumulation = 0 and
    //                                            subframe_index = (a counter advanced per such call) % sppTotal: the raw sample of that index, so that consecutive
    //                                            moving frames do not repeat sample 0's random numbers.  mSubframeIndex stays 0: the first still call starts a
    //                                            normal accumulation.  Not with tile sharing (a raw sample is not gathered).
    // With tile sharing rank 0 makes the call on the gathered image.  params == nullptr: every default.  false: the setting was refused (skh_temporal_check; the
    // previous one stays).  With it off, render() makes the calls it made before.
    bool setTemporal(bool on, const HipTemporal* params = nullptr);
    // what the last render() handed to skh_temporal (false: none yet); hadPrevious: whether that call reprojected a stored history
    bool temporalParams(skh_temporal_params& p, bool* hadPrevious = nullptr) const
    {
        p = mTemporalApplied;
        if (hadPrevious)
            *hadPrevious = mTemporalHadPrevious;
        return mTemporalApplied.width != 0u;
    }
    // Variance guidance (skh_moments + skh_denoise_variance; new), OFF by default.  It acts only when setTemporal and setDenoiser are both on, and only on a call
    // that starts an accumulation (a moving camera's frame).  On such a call skh_temporal writes into an image buffer of this object, with a motion buffer of this
    // object; skh_moments then runs on the raw output image; skh_denoise_variance filters from the object's buffer into the output image with all three flags, in
    // skh_denoise's place.  Two moments buffers change places as the histories do and are dropped whenever the history is.  A call that continues an accumulation
    // makes exactly the calls it makes without the setting and leaves the moments alone.  params == nullptr: every default.  false: the setting was refused
    // (skh_vdenoise_check; the previous one stays).  With it off, render() makes the calls it made before.
    bool setVarianceGuidance(bool on, const HipVariance* params = nullptr);
    // what the last guided render() handed to skh_denoise_variance (false: none yet); hadPrevious: whether that call's skh_moments had previous moments
    bool varianceParams(skh_vdenoise_params& p, bool* hadPrevious = nullptr) const
    {
        p = mVarianceApplied;
        if (hadPrevious)
            *hadPrevious = mMomentsHadPrevious;
        return mVarianceApplied.width != 0u;
    }
    // Object motion (skh_rewind_guides; new), OFF by default.  It acts only with setTemporal on.  With it on, a copy of the instance table as it was last sent to
    // the library is kept beside each of the two guide sets and changes places with them.  A render() that reprojects a stored history compares the two tables'
    // transforms word by word; when they differ it derives the skh_instance_motion table (skh_instance_motion_from_transforms per instance), hands it to
    // skh_set_instance_motion, and makes exactly one skh_rewind_guides call from the current guide set into two more buffers of this object, which then stand
    // in for the normal and position planes of skh_temporal's current frame and, on a guided call, for skh_moments' position plane.  skh_denoise,
    // skh_denoise_variance and the stored guide sets keep the true planes.  With it off -- and on every call that does not reproject across a transform
    // change -- render() makes the calls it made before.
    void setInstanceMotion(bool on);
    // History rectification (skh_rectify; new), OFF by default.  It acts only with setTemporal on, and only on a render() that reprojects a stored history.  On
    // such a call a second skh_temporal call -- the same planes, the rewound ones when setInstanceMotion rewound them; max_history = fastHistory and initial_length
    // min'ed to it; the previous history the stored FAST history; its image output discarded into a buffer of this object -- writes the new fast history, and after
    // the long history's skh_temporal call one skh_rectify call clamps image and long history in place to the fast history's window.  (The fast call comes first:
    // the long one works in place on the raw sample both read.)  skh_moments and the two filters then run on the rectified image as they ran on skh_temporal's.
    // Two fast-history buffers change places as the histories do and are dropped whenever the history is.  A call that continues an accumulation, or starts one
    // without a stored history, makes exactly the calls it makes without the setting: the history it stores is both histories -- the next fast call reads it under
    // its own max_history, which gives it the length min(samples, fastHistory).  params == nullptr: every default.  false: the setting was refused
    // (skh_rectify_check, and a fastHistory that is not finite or < 1; the previous one stays).  The history is dropped by a call that changes the setting (not by
    // turning off what is off); the three buffers are allocated with the guide buffers, by the next guide pass.  With it off, render() makes
    // the calls it made before.  A light change still drops the history (setLightShapes / setEnvironment): keeping it for this pass to correct is the follow-up.
    bool setHistoryRectification(bool on, const HipRectify* params = nullptr);
    // what the last rectifying render() handed to skh_rectify (false: none yet); fastHistory: the max_history of that call's fast skh_temporal call
    bool rectifyParams(skh_rectify_params& p, float* fastHistory = nullptr) const
    {
        p = mRectifyApplied;
        if (fastHistory)
            *fastHistory = mRectifyFastApplied;
        return mRectifyApplied.width != 0u;
    }
    // the frame parameters' sample choice of the last render(): subframe_index and enable_accumulation as handed to skh_render_subframe
    void lastSample(uint32_t& subframeIndex, uint32_t& enableAccumulation) const
    {
        subframeIndex = mLastSubframeIndex, enableAccumulation = mLastEnableAccumulation;
    }

private:
    skh_context* mCtx = nullptr;
    std::string mError;
    uint32_t mWidth = 0, mHeight = 0;
    Mat4 mPrevView{ 0.0f }, mPrevPerspective{ 0.0f };
    // per-instance "previous settings" (function-static in the reference, which makes it non re-entrant:
    // OptixRender.cpp:913,918,923)
    uint32_t mRectLightSamplingMethodPrev = 0, mSppTotalPrev = 0;
    bool mEnableAccumulationPrev = false;
    bool check(skh_status s, const char* what);
    bool applyTiles(uint32_t width, uint32_t height); // this rank's share of the frame -> skh_set_tiles (multi-GPU)
    bool mEnvironmentChanged = false; // render() restarts the accumulation once
    bool mSharing = false;
    int mWorld = 1, mRank = 0;
    uint32_t mTileSize = 32, mMaxTiles = 0;
    std::vector<uint32_t> mAllTileXY; // root: (x0, y0) of every rank's tiles, rank-major, padded to mMaxTiles per rank
    void* mGatherBuf = nullptr; // root: [world][mMaxTiles][tile^2] float4
    void uploadScene(); // mFrameNumber == 0 block: OptixRender.cpp:876-888
    // instances the scene marks dirty (Scene::updateInstanceTransform) whose transform differs from what was last sent: the whole table goes to
    // skh_update_accel (in place where it can); true = something was sent
    bool sendMovedInstances();
    std::vector<skh_instance> mSentInstances;
    bool mAlphaBlend = false;
    bool mAdaptive = false, mConverged = false;
    skh_adaptive mAdaptiveSetting = {}, mAdaptiveApplied = {}; // (dark_level of the setting: the RADIANCE; of the applied one: the LDR level)
    float mAdaptiveDarkRadiance = 0.0f;
    std::vector<skh_light_shape> mLightShapes; // setLightShapes' table, re-applied after skh_set_lights
    bool mLightsUploaded = false, mLightShapesChanged = false;
    bool applyLightShapes();
    bool mDenoise = false;
    HipDenoise mDenoiseSetting;
    skh_denoise_params mDenoiseApplied = {};
    void* mGuide[4] = {}; // ids | normal | position | albedo of the whole image, through the pixel centres
    uint32_t mGuideWidth = 0, mGuideHeight = 0;
    bool mGuidesValid = false;
    float mSceneDiagonal = 0.0f; // of the mesh instances' bounding box (uploadScene, sendMovedInstances)
    void measureScene(const std::vector<skh_instance>& inst);
    bool renderGuides();
    void freeGuides();
    bool mTemporal = false;
    HipTemporal mTemporalSetting;
    skh_temporal_params mTemporalApplied = {};
    bool mTemporalHadPrevious = false;
    void* mHistory[2] = {};    // {illumination.rgb, n} per pixel; mHistory[mHistoryStored] is the stored one, the other the next call's output
    int mHistoryStored = 0;
    bool mHistoryValid = false; // false: the next call has no previous frame
    void* mPrevGuide[3] = {};  // ids | normal | position the stored history belonged to when the guide sets last changed places
    bool mPrevGuidesValid = false;
    float mGuideWorldToClip[16] = {}, mPrevWorldToClip[16] = {}; // of mGuide / mPrevGuide
    uint32_t mRotation = 0;    // moving start calls so far (rotateSamples)
    bool mRendered = false;    // a render() has been made: mPrevView is a camera
    uint32_t mLastSubframeIndex = 0, mLastEnableAccumulation = 0;
    bool mVariance = false;
    HipVariance mVarianceSetting;
    skh_vdenoise_params mVarianceApplied = {};
    bool mMomentsHadPrevious = false;
    void* mVarianceImage = nullptr; // skh_temporal's image output on a guided call: skh_denoise_variance's input
    void* mMotion = nullptr;        // skh_temporal's motion plane on a guided call
    void* mMoments[2] = {};         // {mu1, mu2, variance, nm} per pixel; mMoments[mMomentsStored] is the stored one
    int mMomentsStored = 0;
    bool mMomentsValid = false;     // false: the next guided call has no previous moments
    bool mInstanceMotion = false;
    std::vector<skh_instance> mGuideInstances, mPrevGuideInstances; // the instance table as sent when mGuide / mPrevGuide were rendered (setInstanceMotion)
    void* mRewound[2] = {};  // position | normal of mGuide in the previous frame's world (skh_rewind_guides' outputs)
    bool rewindGuides(uint32_t width, uint32_t height); // true: mRewound holds this call's rewound planes
    bool mRectify = false;
    HipRectify mRectifySetting;
    skh_rectify_params mRectifyApplied = {};
    float mRectifyFastApplied = 0.0f;
    void* mFast[2] = {};            // the fast history, {illumination.rgb, n} per pixel; mFast[mFastStored] is the stored one
    int mFastStored = 0;
    bool mFastValid = false;        // false: the stored long history is the fast one too (a continued accumulation, a first frame)
    void* mRectifyImage = nullptr;  // the fast skh_temporal call's image output: discarded
    // the fast history's skh_temporal call for the temporal call `tp` on the raw image dColor; true: mFast[1 - mFastStored] holds this frame's fast history (not yet the stored one)
    bool fastHistory(const skh_temporal_params& tp, const void* dColor, const void* normal, const void* position);
    // after the long history's call succeeded: that fast history becomes the stored one, and skh_rectify runs in place on dImage and dHistory (what the long call wrote)
    void rectifyHistory(const skh_temporal_params& tp, void* dImage, void* dHistory);
    void dropHistory()
    {
        mHistoryValid = false;
        mMomentsValid = false;
        mFastValid = false;
    }
    void uploadMaterials(); // MaterialDescription list -> skh_material blocks + textures (OptixRender.cpp:1270-1433)
};

} // namespace oka
