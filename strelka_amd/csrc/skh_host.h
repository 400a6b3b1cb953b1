// skh_host.h -- what the host-side files of the library's one translation unit share (strelka_hip.hip and skh_accel.inc): the owning device
// buffer, the context, the two status macros and the allocation helpers.
#pragma once
#include "../../include/strelka_hip.h"
#include "skh_kernels.h"
#include "skh_order.h"
#include "skh_stale.h"

#include <string>
#include <utility>
#include <vector>

typedef struct ncclComm* ncclComm_t; // (RCCL is loaded at run time: strelka_hip.hip)
using namespace skh;

namespace
{
// A device allocation and its owner: freed when it goes out of scope, handed on by move / std::swap, never copied.
struct DevBuf
{
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes)
    {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept // (frees what it held)
    {
        if (this != &o)
        {
            reset();
            p = o.p, bytes = o.bytes;
            o.p = nullptr, o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf()
    {
        reset();
    }
    void reset()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as() const
    {
        return reinterpret_cast<T*>(p);
    }
};

enum KernelClass
{
    KC_TRACE_CLOSEST = 0,
    KC_TRACE_SHADOW,
    KC_SHADE,
    KC_RAYGEN,
    KC_ACCUM,
    KC_SORT,
    KC_AOV, // skh_render_aovs: its ray generation, trace launches and resolve (in no field of skh_stats)
    KC_COUNT
};

#ifndef SKH_RI_MAX_LEVELS
#define SKH_RI_MAX_LEVELS 1024 // per-level counters of the reinsertion pass's refit: a ring (a deeper tree wraps around it; tests build a variant with 3)
#endif
#define SKH_MAX_LAUNCH_ROUNDS 140 // MAX_BOUNCES (128) + slack

struct TimedSpan
{
    int cls;
    hipEvent_t a, b;
};
} // namespace

// The context: one member struct per subject, every member in exactly one of them.  `scene` is what the skh_set_* calls stored, `opt` what skh_set_option stored;
// everything else is derived from those two -- `accel` by the builders, the feature groups (`env`, `emit`, `mtex`, `cut`, `lshape`) by their setters and
// *_ensure functions, `frame` by alloc_frame -- or is state of the calls in progress (`spec`, `adapt`, `timing`, `aov`, `dn`, `tp`).  Which change of an input
// invalidates which derived state: skh_stale.h.  No group is ever reset wholesale while the context lives, except `adapt` by skh_set_adaptive(NULL): the
// buffers are kept and reused by dev_alloc's size window.
struct skh_context
{
    // ---- device and streams ----
    struct Device
    {
        int device = 0;
        hipStream_t stream = nullptr;
        hipStream_t stream2 = nullptr; // any-hit launches when `overlap` is on: shadow[b] runs beside closest[b+1] and fills its tail
        hipStream_t stream3 = nullptr; // accumulation steps + image copies beside a pass in flight (non-blocking: no implicit sync with the null stream)
        hipEvent_t evShade = nullptr, evShadow = nullptr;
        int numCUs = 256;
        uint32_t* hOverflow = nullptr; // pinned, device-visible: traversal-stack overflow flag (DevScene::overflowFlag)
        std::string err;
    } dev;

    // ---- multi-GPU: the tile gather (skh_comm_init) and scatter ----
    struct MultiGpu
    {
        ncclComm_t comm = nullptr;
        int world = 1, rank = 0;
        DevBuf dTileSend, dScatterXY;
    } multi;

    // ---- scene inputs: what the skh_set_* calls store (the per-material and per-light tables of the features are kept with the feature) ----
    struct Scene
    {
        // host copies needed for the build, counts, the input device buffers
        std::vector<skh_mesh> meshes;
        std::vector<skh_curve> curves;
        std::vector<uint32_t> curveVertexCounts;
        std::vector<skh_instance> instances;
        std::vector<int32_t> lightTypes; // of the light list, kept for the light shapes' derivation
        uint32_t nVerts = 0, nIndices = 0, nPoints = 0, nInstances = 0, nLights = 0, nMaterials = 0;
        DevBuf dVerts, dIndices, dMeshes, dPoints, dRadii, dInstances, dLights, dMaterials, dHairConst;
        // signatures of the TOPOLOGY (FNV-1a over the words): of the mesh table + index buffer, and of the curve sets' table + vertex counts.  The in-place
        // updates keep a hierarchy only while these are the built ones (accel.builtGeomSig, accel.builtCurveSig)
        uint64_t geomSig = 0, curveSig = 0;
        DevBuf dTexels, dTexDesc;
        uint32_t nTextures = 0;
        bool hasHairMaterial = false; // selects the k_shade build that carries df::chiang_hair_bsdf
    } scene;

    // ---- options: exactly what the rows of kOptions store (skh_set_option), with what was measured when each default was chosen ----
    struct Options
    {
        bool countTraversal = false, timing = false;
        int overlap = 1; // 0 off, 1 for small passes only (<= 8 M paths: the interactive one-sub-frame-per-call mode, +7 %), 2 always
        uint32_t speculateAsync = 1; // option speculate_async: 224 -> 180 ms per frame in the reference caller's loop with map() (docs/LOG.md)
        uint32_t speculateGrow = 2; // option speculate_grow: how fast the look-ahead grows while the caller keeps continuing a frame (x2 per pass: 2, 4, 8; 8 = straight to the cap at the second call)
        uint32_t speculateMax = 8; // option "speculate": most sub-frames traced ahead in one pass (0 / 1 = off).  8: a pass stays below ~25 ms at 1080p
        uint32_t envNee = 1, emitNee = 1; // options env_nee, emit_nee
        uint32_t cutoutRounds = 8; // option cutout_rounds
        uint32_t aovBand = 1u << 22; // option aov_band: rays per band
        int32_t fetchChunk = -1; // option fetch_chunk: queue positions a trace wave reserves per atomic; 0 = one atomic per refill; -1 = automatic
        // scheduling of the persistent trace kernels, measured on MI355X (kitchen C3, 32 sub-frames per pass):
        uint32_t wavesPerCU = 28; // resident waves per CU (7 per SIMD at <= 72 VGPRs; the curve build is resident 16 at a time whatever is asked: 128 VGPRs)
        uint32_t wavesPerCUShadow = 28; // the any-hit build of the triangle kernel fits 7 per SIMD
        uint32_t wavesPerCUShadowWorld = 32; // ... its world-only build 8 (SKH_WORLD_ANYHIT_MIN_WAVES)
        uint32_t wavesPerCUWorld = 32; // the world-only closest-hit build: 64 VGPRs, 8 per SIMD (SKH_WORLD_CLOSEST_MIN_WAVES)
        uint32_t smallWavesClosest = 0, smallWavesShadow = 0; // (0 = automatic: 20 / 12 for triangle scenes, 16 / 16 with curves -- there the any-hit launch is the heavier one: hair 1-spp calls 687 against 664 Mray/s) overlapped (small) passes: waves per CU of each of the two concurrent trace kernels (0 = wavesPerCU); 16/16: +4 % on 1-spp 1080p launches over 24/24; round 6: the closest-hit launch is the one on the critical path -- 20/12: 1-spp 1080p calls 3.49 -> 3.39 ms, drop-in +1 % (18/14 3.41, 22/10 3.48, 24/8 3.67: then the any-hit launch is the long one)
        uint32_t fetchMinClosestSmall = 48; // option fetch_min_closest_small
        uint32_t smallWavesFirst = 0, smallWavesLast = 0; // (small overlapped passes) waves per CU of the FIRST closest-hit launch and of the LAST any-hit launch, which have the machine to themselves; 0 = as the others, except that the last any-hit launch of a triangle scene takes 20 of 32 instead of 12 (1-spp 1080p call 3.13 -> 3.10 ms; 16 / 24 the same, 32: 3.13; the first closest-hit launch at 24 / 28 / 32: 3.12 / 3.13 / 3.15)
        int tailSplit = 1; // option tail_split: 1 (default) = the world-only triangle kernels' SPLIT build for every launch of a scene whose hierarchy has more than 16 384 nodes -- once a wave finds the ray queue dry (the tail
                           // phase of k_trace: skh_trace_body.inc included a second time), its idle lanes take stack entries of the lanes that still hold a ray --, 2 = for every launch whatever the hierarchy (tests), -1 = for passes
                           // of 2^17 ... 2^23 paths only, 0 = never.  Per launch 285 + 274.5 n -> 225 + 272.9 n us (closest-hit, n sub-frames of 2.07 M paths), 228 + 115.0 n -> 148 + 114.8 n (any-hit): the main phase is the plain
                           // build's, instruction for instruction.  Hierarchies that fit the L2 many times over (Cornell: 30 triangles, rays of two or three steps) have no tails to speak of and lose by the hand-out:
                           // closest-hit 27.6 -> 28.4 ms with it (the same scenes whose launches are bound by the queue cursors: fetch_chunk)
        uint32_t fetchMinClosest = 32 /* 24 until round 5: on the reinserted trees 32 is 0.4 ... 0.9 % ahead on all three kitchens, gpurun_out/r6c */, fetchMinShadow = 48; // idle lanes before a wave pulls new rays from the queue (round 3, world-space hierarchy: any-hit 32 -> 48: 39.7 -> 36.2 ms, 56: 37.5, 64: 51; closest 12..40 within 1 %)
        bool fetchMinClosestSet = false; // fetch_min_closest was set explicitly
        uint32_t curveFetchMinClosest = 16, curveFetchMinShadow = 16 /* 24 until the result writes got cheaper (round 5, late): hair any-hit 47.5-47.8 -> 46.5-47.0 ms with 12 ... 20, gpurun_out/r7v */, curveNodeBreakClosest = 20, curveNodeBreakShadow = 20; // the same four for the curve build (6 waves/SIMD): hair 482 vs 465 Mray/s
        uint32_t nodeBreakClosest = 32, nodeBreakShadow = 28; // (closest: 24 -> 32 in round 3 for the world-only kernel: kitchen 86.6 -> 85.9 ms, unshared 74.7 -> 73.6, three runs each;
                                                              // shadow: 20 -> 28 in round 4, with the shared triangle pass: kitchen 34.85 -> 34.3 ms, unshared 29.3 -> 28.55, three runs each; 36: 34.35 / 28.7)
        // leave the node loop when fewer than x/64 of the wave's rays are still descending
        uint32_t worldCurveMin = 32; // ... of the world-only kernel with the curve block (option curve_min sets both)
        uint32_t curveMin = 48; // (cooperative curve block) end-point runs queued by the parked lanes before the block runs, one run per lane (round 3, Mray/s on the hair
                                // stand-in: 16: 712, 32: 907, 40: 958, 48: 984, 56: 971, 64: 887; round 2 counted parked LANES whose owners ran their own runs: 48: 334)
        uint32_t leafMin = 16; // postpone the minority kind of leaf work unless it has this many lanes (0 = never postpone; measured +1.5 % at 16)
        uint32_t subframeBatch = 0; // option subframe_batch: 0 = auto (frame.batchCapacity)
        uint32_t queueOrder = 1; // option queue_order: where k_raygen puts a pass's camera rays in the first queue (skh_order.h).  0 = slot order, sub-frame after sub-frame; 1 = cell by
                                 // cell, all sub-frames of a cell together.  A pass of one sub-frame is the same under both
        int32_t cellBlocks = 0;  // option cell_blocks: 512-slot raygen blocks per cell of queue_order 1; -1 = an eighth of a block (one 64-slot chunk, a wave of k_raygen); 0 = automatic
        bool worldKernel = true; // option world_kernel: scenes with an empty top level run the world-only build of k_trace (0 = the general build: A/B, tests)
        // -- what skh_build_accel reads --
        uint32_t reinsertRounds = 8; // option reinsert_rounds: rounds of parallel reinsertion over the PLOC tree of the triangle build (skh_bvh.h k_ri_*)
        uint32_t reinsertCurveRounds = 4; // option reinsert_curve_rounds: the same pass over the curve sub-segment trees
        uint32_t reinsertMinSize = 0; // option reinsert_min_size: 0 = auto (1 up to 4 M primitives, 32 beyond)
        uint32_t plocTop = 0; // triangle build: clusters left at which PLOC switches to the wide neighbour search (option ploc_top; 0 = never)
        bool tightInstanceBoxes = true; // TLAS leaf boxes from the transformed vertices, not from the transformed object box
        uint32_t curveLeaf = 1; // sub-segments per curve leaf (option curve_leaf; hair stand-in after the intersector's early exit, Mray/s: 1: 1456, 2: 1392, 3: 1309, 4: 1240;
                                // the cooperative block takes two candidates per lane and block)
        uint32_t splitPairs = 0; // (option split_pairs, tenths) triangle trees: a two-triangle subtree whose box exceeds this x the summed areas of its triangles' boxes may be opened into two one-triangle leaves (0 = off)
        uint32_t curveMerge = 1; // (option curve_merge) curve instances under identity transforms share ONE world-space tree in the world-only curve kernel
        uint32_t curveSegNode = 0; // (option curve_segnode) 1: the curve tree is built over whole segments and ends in SEGMENT NODES (skh_bvh.h k_segnode_emit): a segment is a
                                   // candidate at most once per ray; 0: parameter sub-ranges as primitives (curve_split), rounds 3-5
        uint32_t curveStrandMajor = 0; // (option curve_strand_major, segment-node build) 1: leaf records and segment nodes at the segment's own index (consecutive segments of a strand adjacent)
        uint32_t curveSplit = 4; // parameter sub-ranges per curve segment in the curve BLAS (round 3, one-sub-segment leaves: 2: 1460, 3: 1480, 4: 1503 Mray/s; build time and leaf
                                 // memory grow with it.  Round 2, ms per 1080p sub-frame: 1: 61.6, 2: 52.1, 4: 49.7, 8: 50.1)
        // TLAS builder.  1 (default): on the GPU -- PLOC over the instance boxes with a 96-neighbour search, the BLAS builder, no host round
        // trip: 4 / 5 / 9 ms for 2 k / 20 k / 100 k instances.  0: exact three-axis sweep SAH on the host, O(n log^2 n) single-threaded
        // (4 / 45 ms for 2 k / 20 k), whose tree enters 5 % fewer instances (1.28 vs 1.35 per ray on the kitchen stand-in with only its
        // room baked: closest-hit 97.6 vs 100.3 ms; PLOC radius 24 .. 512 makes no difference, docs/LOG.md).  With bake_world 4 a top level
        // only exists for curve sets, for light proxies beside them, and for scenes with more than bake_budget_mtris instanced triangles:
        // every structure the bench workloads traverse is built by GPU kernels.  2: the sweep up to 8192 TLAS leaves, the GPU beyond.
        uint32_t tlasBuild = 1;
        uint32_t tlasOpen = 1; // TLAS opening: up to tlasOpen x numInstances leaves; 1 = one leaf per instance (default: on the kitchen stand-in 2..16 were 4-9 % slower, more instance entries for no fewer nodes)
        // bake_world: mesh instances that skip the TLAS -- their triangles are carried to world space once and join ONE extra
        // group of the triangle build that every ray walks first, with no instance entry (DESIGN.md section 2 "bake_world").
        // 0 off; 1: instances whose mesh has a single user (what HdStrelka's per-instance meshes are, RenderPass.cpp:126-129,252-257);
        // 2: also instances of meshes with <= bakeSmallTris triangles (room shells, boards, quads: big boxes that every ray enters
        // for a dozen triangles), while they add at most max(unique triangles, 2^20) triangles
        uint32_t bakeWorld = 4, bakeSmallTris = 64, bakeBudgetMTris = 64;
        uint32_t mortonBits = 10; // per axis, in the builders' sort keys (option morton_bits 4..21: 10 / 13 / 16 / 20 measured within the +-1.5 % the tree's shape varies by anyway)
        uint32_t leafLines = 0;   // 1: triangle leaves laid out by 128-byte line (skh_bvh.h: k_leaf_place): -11 % fetched lines, same time (docs/LOG.md)
        uint32_t mergeLightProxies = 0; // option merge_light_proxies: baked light proxies share the world-space mesh triangles' tree (any-hit queries skip their triangles) instead of a tree of their own that every radiance ray visits (a measured loss: docs/LOG.md round 5)
        int32_t directRecords = -1; // option direct_records: -1 = by the counts (accel.directRecords), 0 / 1 forced
        uint32_t compactHits = 1;   // option compact_hits: 16-byte hit records in the render passes of world-only triangle scenes that fit (HitQ::primBits)
        uint32_t leafMaxTris = 2; // measured on MI355X: 2 beats 1, 3, 4, 6, 8 (the kernel is ALU bound, wasted triangle tests cost more than extra nodes)
        uint32_t buildQuality = 1; // 0: Karras radix tree (fastest build), 1: PLOC clustering (SAH-class quality)
    } opt;

    // ---- acceleration structures: what skh_build_accel, skh_update_accel and skh_refit_accel produce or keep for each other, and what make_dev_scene,
    // trace_build and launch_trace read from a build ----
    struct Accel
    {
        bool built = false; // the hierarchies are those of the scene inputs (skh_stale.h D_ACCEL_BUILT)
        DevBuf dTriNodes, dTris, dSegNodes, dSegs, dTlasNodes, dTlasInst, dDevInst, dTravInst;
        DevBuf dShadeTris, dShadeInst; // shading side: de-indexed triangle records, instance records that carry their mesh's base
        DevBuf dCurveSegBase, dSegStartAll;
        int tlasRoot = SKH_REF_INVALID;
        int worldRoot = SKH_REF_INVALID, lightRoot = SKH_REF_INVALID; // roots of the two baked groups (mesh instances, light proxies) inside dTriNodes
        uint32_t nTris = 0, nSegs = 0;
        uint32_t nTriSlots = 0;
        uint32_t hierNodes = 0; // 4-wide nodes of the triangle and curve trees: decides the automatic fetch_chunk
        uint32_t numTlasLeaves = 0;
        uint32_t curveSplitBuilt = 1;
        uint32_t numWorldCurves = 0; // curve instances under identity transforms that the world-only kernel walks itself
        int worldCurveRoot[SKH_WORLD_CURVES];
        uint32_t worldCurveInst[SKH_WORLD_CURVES];
        uint32_t worldCurveMerged = 0; // bit k: table entry k is a merged transform group (its hits take their instance from the segment record)
        uint32_t worldCurveIdentLast = 0;
        uint32_t numMergedCurveInst = 0; // curve instances that share the merged world-space tree
        std::vector<uint8_t> baked; // per instance, valid after skh_build_accel
        uint32_t nBakedTris = 0, nBakedInst = 0;
        LightBox lightBox = { { -INFINITY, -INFINITY, -INFINITY }, { INFINITY, INFINITY, INFINITY } }; // around the baked light proxies' group, with the node encoder's margin
        uint32_t nShadeRecords = 0; // de-indexed shading triangle records (build_shading_tables)
        uint32_t directRecords = 1; // baked mesh triangles name their shading record (SKH_PRIM_DIRECT); 0 when only (instance, mesh-local primitive) fits a 16-byte hit record
        uint32_t hitPrimRange = 0;  // primitive words of this scene's hits stay below it (records, or mesh-local indices; curve segments)
        skh_build_info buildInfo = {};
        double msBuild = 0.0;
        // skh_refit_accel: what the last build leaves behind for it -- the triangle tree's leaf order and primitive tables (k_gather_tris' inputs), the
        // nodes' levels -- and what must not have changed since (the signature of the mesh table + index buffer, the vertex count)
        bool refitReady = false;
        DevBuf dTriOrder, dTriMeshK, dTriLocalK, dWInstK, dWFirstK, dTriNodeBox;
        std::vector<uint32_t> triLevelStart;
        uint32_t nMeshTrisBuilt = 0, nWInstBuilt = 0, triNumNodes = 0, lastBuildFlags = 0, nMeshGroupsBuilt = 0, nGroup1Built = 0;
        uint64_t builtGeomSig = 0;
        uint32_t builtNVerts = 0;
        double msRefit = 0.0;
        uint32_t refits = 0;
        // ... and of the curve build: k_gather_segs' tables, the curve tree's levels, the signature of the curve sets' topology (control points and radii may change)
        DevBuf dSegOrder, dSegBuildStartK, dSegLocalK, dSegInstOfK, dSegNodeBox;
        std::vector<uint32_t> segLevelStart;
        uint32_t nSubBuilt = 0, segNumNodes = 0;
        uint64_t builtCurveSig = 0;
        bool curvePointsEdited = false, curveRefitReady = false;
        // skh_update_accel (edited instance transforms, any scene kind): what the last build leaves behind for it -- the instance table it was built from (kept
        // up to date by every update), per instance whether its transform had a finite inverse and whether it took a TLAS leaf, the BLASes' group roots and
        // bounds (k_instance_boxes' inputs), the TLAS's node levels, the merged curve groups -- and the instance boxes' scratch
        bool updateReady = false; // the last skh_build_accel ran to its end
        bool vertsEdited = false; // skh_set_geometry since the last build / refit / update
        std::vector<skh_instance> builtInstances;
        std::vector<uint8_t> builtInvOk;
        std::vector<std::vector<uint32_t>> builtMergedGroups;
        DevBuf dBuiltValid, dW2o, dInstLo, dInstHi, dInstGrp, dTriGroupRoot, dTriGroupBounds, dSegGroupRoot, dSegGroupBounds, dTlasNodeBox;
        std::vector<uint32_t> tlasLevelStart;
    } accel;

    // ---- environment light (skh_set_environment): w != 0 selects the k_shade build that carries it ----
    struct Environment
    {
        DevBuf dTexels, dColCdf, dRowCdf;
        uint32_t w = 0, h = 0;
        float scale[3] = { 1.0f, 1.0f, 1.0f }, w2e[9] = { 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f };
        double sumW = 0.0, msBuild = 0.0;
    } env;

    // ---- emissive meshes (skh_set_emission): the per-material radiances as the caller gave them, and the emitter table derived from them, the geometry, the
    // instances and the material count (emit_ensure builds it when stale).  sumW > 0 selects the k_shade build that carries it. ----
    struct Emitters
    {
        std::vector<float> emission; // 3 per material; empty: nothing emits
        bool stale = false;
        DevBuf dEntries, dCdf, dGuide, dLe, dInstOffset;
        uint32_t count = 0, instances = 0, guideBits = 0;
        double sumW = 0.0, msBuild = 0.0;
    } emit;

    // ---- material textures (skh_set_material_textures): the table as the caller gave it and its device copy.  mtex_active() -- an entry binds a texture that
    // exists -- selects the k_shade build that carries it. ----
    struct MaterialTextures
    {
        std::vector<skh_material_textures> table;
        DevBuf dTable;
    } mtex;

    // ---- cutouts and fractional opacity: one group, they share cut_ensure and the stage's buffers ----
    struct Cut
    {
        // cutouts (skh_set_material_cutouts): the table as the caller gave it and its device copy.  Whether a cutout is IN USE -- an active entry on a material that a mesh
        // instance uses -- is derived (cut_ensure, when stale): only then does the cutout stage run, and only then do its buffers exist: two continuation queues and a
        // second hit buffer for the closest-hit side, the same plus the first-round hit buffer for the shadow side (the two sides run on two streams when `overlap` is on)
        std::vector<skh_material_cutout> cutouts;
        DevBuf dCutouts, dStats, dQ[2], dHits, dShadowQ[2], dShadowHits[2];
        bool stale = false;
        uint32_t activeMaterials = 0, instances = 0; // instances != 0: a cutout is in use
        // fractional opacity (skh_set_material_blend): the table as the caller gave it and its device copy, one packed uint4 per material (BlendP).  Whether blending is IN
        // USE is derived with the cutouts' (cut_ensure): the stage runs -- and its buffers exist -- when a cutout OR a blend entry is in use (cut_stage_on); its BLEND build
        // is launched only when a blend entry is
        std::vector<skh_material_blend> blends;
        DevBuf dBlend;
        uint32_t blendActiveMaterials = 0, blendInstances = 0; // blendInstances != 0: blending is in use
    } cut;

    // ---- light shapes (skh_set_light_shapes): the table as the caller gave it.  Which entries are IN USE -- a flag that applies to its light's type, inside the light
    // list -- is derived (lshape_ensure, when stale): the device table holds one entry per light with the flags masked to those, and exists only when one is
    // in use; only then do the k_shade builds with LSHAPE in them run ----
    struct LightShapes
    {
        std::vector<skh_light_shape> table;
        DevBuf dTable;
        bool stale = false;
        uint32_t discs = 0, cones = 0;
    } lshape;

    // ---- frame: size, tiles, slots, the frame buffers, the ray-generation tables, what alloc_frame derives from the options ----
    struct Frame
    {
        uint32_t width = 0, height = 0, tileSize = 32, tileShift = 5, numTiles = 0, numSlots = 0;
        std::vector<uint32_t> tileXY;
        bool customTiles = false;
        DevBuf dTileXY, dAccum, dDiffuse, dSpecular, dDiffCnt, dSpecCnt, dSums, dPath, dRayQ[2], dHits, dShadowQ, dContrib, dCounts, dOvf, dOvf2, dScratchImage;
        DevBuf dRaygenBase;
        uint32_t raygenBlocksPerSub = 0, raygenValidPerSub = 0;
        // queue_order 1: k_raygen's tables of the cell order (skh_order.h), per pass size -- they depend on `batch` --, cell size and tile set; built by the first pass that
        // needs them (raygen_order).  alloc_frame drops them; an adaptive pass's are those of the frozen set numbered adapt.orderGen
        struct CellTables
        {
            uint32_t batch = 0, gen = 0;
            int32_t cellBlocks = 0;
            bool adaptive = false;
            DevBuf dQBase, dSubStride;
        };
        std::vector<CellTables> cellTables;
        uint32_t cellTablesNext = 0; // the entry the next new key overwrites once the few there are hold other keys
        std::vector<uint32_t> chunkValid; // valid pixels per 64-slot chunk (an 8 x 8 pixel block) of the home list: what the ray-generation tables are summed from
        uint32_t queueConstBits[2] = { 0, 0 }; // materialTmin / shadowTmin the constant planes of the ray queues hold (bit patterns)
        bool queueConstFilled = false; // ... and whether they hold them at all (alloc_frame resets it)
        uint32_t batchCapacity = 1; // sub-frames a wavefront pass holds (option subframe_batch, or by the frame's size)
        uint32_t queueRegion = 64; // positions per queue shard (RayQ::region): the queues hold SKH_SHARDS * queueRegion rays
        uint32_t traceBlocks = 0;
    } frame;

    // Speculative sub-frame batching for the reference's call pattern (one render() per sub-frame, RenderPass.cpp:441-447): once two
    // consecutive calls continue the same frame (same parameters, subframe_index + 1), the next call traces several sub-frames
    // ahead in ONE wavefront pass and the calls after it only apply their accumulation step to the radiances already in the path
    // state.  Exact (sub-frame batching is exact); a call that does not continue the frame discards what is left.
    struct Speculation
    {
        bool valid = false;
        skh_frame_params params; // of the pass (subframe_index = its first sub-frame)
        uint32_t count = 0, consumed = 0, lastBatch = 1, streak = 0;
        skh_frame_params last; // the previous call's parameters
        bool haveLast = false;
        uint64_t passRadiance = 0, passShadow = 0; // rays the pass traced (all `count` sub-frames; counted when traced)
        // option speculate_async: the pass AFTER the one being consumed is already being traced -- on dev.stream, into the other
        // path-state buffer -- while the caller collects this pass's sub-frames (accumulation steps and map() copies on stream3)
        uint32_t buf = 0; // path-state buffer of the pass being consumed (0 = frame.dPath, 1 = dPathB)
        bool nextInFlight = false;
        skh_frame_params nextParams;
        uint32_t nextCount = 0;
        unsigned long long statsMark[2] = { 0, 0 }; // timing.dStats {raysRadiance, raysShadow} when the pass in flight was launched
        DevBuf dPathB;
        uint32_t pathBStride = 0;
        // sub-frames traced ahead and then thrown away (camera move, a setter, resize): their rays are taken out of the ray counts again,
        // so that a Mray/s figure from skh_get_stats only counts rays whose sub-frame was delivered
        uint64_t discardedRadiance = 0, discardedShadow = 0;
        uint32_t discardedSubframes = 0;
    } spec;

    // adaptive sampling (skh_set_adaptive; skh_adapt.h).  Nothing below exists in a context that never turned it on.  A pass of an adaptive call takes the
    // RENDER tile list -- the context's list with the frozen tiles' origins moved off the image -- and the ray-generation tables computed for it, where it
    // otherwise takes frame.dTileXY / dRaygenBase / raygenValidPerSub; read-back, tile copies and the gather keep the home list.
    struct Adaptive
    {
        bool on = false;
        skh_adaptive cfg = {};
        bool ready = false;      // buffers allocated for this frame geometry and the frame's state initialised (cleared by every reset)
        uint32_t delivered = 0;  // observations since the frame began
        uint32_t checks = 0, activeTiles = 0, raygenValid = 0;
        uint32_t orderGen = 0; // counts the frozen sets: frame.cellTables of an older one are stale
        uint64_t pixelObs = 0, pixelObsSaved = 0;
        std::vector<uint32_t> frozenAt; // per tile: 0 = active, else its observation count when it froze
        DevBuf dTileXYRender, dRaygenBaseRender, dState, dTileQ, dFrozenAt;
    } adapt;

    // ---- timing and counters: what skh_get_stats reports beside the rays ----
    struct Timing
    {
        std::vector<TimedSpan> spans;
        std::vector<hipEvent_t> eventPool;
        size_t eventsUsed = 0;
        double msClass[KC_COUNT] = { 0, 0, 0, 0, 0, 0, 0 };
        uint32_t launches[KC_COUNT] = { 0, 0, 0, 0, 0, 0, 0 };
        DevBuf dStats; // StatsDev: the kernels' ray and traversal counters (DevScene::profile)
        uint32_t stackOverflows = 0; // calls that failed with the traversal-stack overflow flag set since the last skh_reset_stats
    } timing;

    // first-hit AOVs (skh_render_aovs): nothing but this lives between two calls
    struct Aov
    {
        skh_aov_info info = {};
    } aov;

    // the denoiser (skh_denoise; skh_denoise.h): its scratch -- two colour images and the packed guide record -- exists from the first call until
    // skh_denoise(ctx, NULL, ...) or skh_destroy
    struct Denoiser
    {
        DevBuf dColor[2], dG0, dG1;
        skh_denoise_info info = {};
    } dn;

    // temporal accumulation (skh_temporal; skh_temporal.h): no scratch, nothing but this lives between two calls
    struct Temporal
    {
        skh_temporal_info info = {};
    } tp;

    // variance guidance (skh_moments, skh_denoise_variance; skh_variance.h): the filter's scratch is the denoiser's, nothing but this lives between two calls
    struct Moments
    {
        skh_moments_info info = {};
    } mo;
    struct VarianceDenoiser
    {
        skh_vdenoise_info info = {};
    } vd;

    // object motion (skh_set_instance_motion, skh_rewind_guides; skh_motion.h): the table is an input of its own -- no scene setter touches it, and it is no
    // entry of skh_stale.h.  It exists from a set with n > 0 until a set with n == 0 or skh_destroy.
    struct Motion
    {
        DevBuf dTable;
        uint32_t entries = 0;
        skh_rewind_info info = {};
    } rw;

    // history rectification (skh_rectify; skh_rectify.h): no scratch, nothing but this lives between two calls
    struct Rectify
    {
        skh_rectify_info info = {};
    } rc;
};

// A caller changed `in`: every derived state that depends on it is invalidated (the table: skh_stale.h).
static inline void touched(skh_context* c, skh_stale::Input in)
{
    using namespace skh_stale;
    bool* flag[D_COUNT] = {};
    flag[D_ACCEL_BUILT] = &c->accel.built, flag[D_REFIT_READY] = &c->accel.refitReady, flag[D_UPDATE_READY] = &c->accel.updateReady;
    flag[D_VERTS_EDITED] = &c->accel.vertsEdited, flag[D_CURVE_POINTS_EDITED] = &c->accel.curvePointsEdited;
    flag[D_EMIT_STALE] = &c->emit.stale, flag[D_CUT_STALE] = &c->cut.stale, flag[D_LSHAPE_STALE] = &c->lshape.stale;
    apply(in, flag);
}

// a failing HIP call ends the function: its message names the function, the call and the HIP error
#define SKH_TRY(ctx, expr)                                                                                              \
    do                                                                                                                  \
    {                                                                                                                   \
        hipError_t _e = (expr);                                                                                         \
        if (_e != hipSuccess)                                                                                           \
        {                                                                                                               \
            (ctx)->dev.err = std::string(__func__) + ": " #expr ": " + hipGetErrorString(_e);                          \
            return _e == hipErrorOutOfMemory ? SKH_OUT_OF_MEMORY : SKH_FAIL;                                           \
        }                                                                                                               \
    } while (0)
// ... and so does a callee's status other than SKH_OK (the callee left the message)
#define SKH_CHECK(expr)                                                                                                 \
    do                                                                                                                  \
    {                                                                                                                   \
        const skh_status _s = (expr);                                                                                   \
        if (_s != SKH_OK)                                                                                               \
            return _s;                                                                                                  \
    } while (0)

static skh_status dev_alloc(skh_context* c, DevBuf& b, size_t bytes)
{
    if (b.p && b.bytes >= bytes && b.bytes <= bytes * 2 + 4096)
        return SKH_OK;
    b.reset();
    if (bytes == 0)
        bytes = 16;
    SKH_TRY(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return SKH_OK;
}
static skh_status dev_upload(skh_context* c, DevBuf& b, const void* src, size_t bytes)
{
    SKH_CHECK(dev_alloc(c, b, bytes));
    if (bytes)
        SKH_TRY(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->dev.stream));
    SKH_TRY(c, hipStreamSynchronize(c->dev.stream));
    return SKH_OK;
}
static void dev_free(DevBuf& b) // (a buffer dropped on purpose before its scope ends)
{
    b.reset();
}
