"""Entry points of include/strelka_hip.h that no other GPU test calls directly: ray queries on caller-owned device arrays
(skh_trace_device), the device description bench.py prices its roofs with (skh_get_device_info), the context stream handle
(skh_get_stream) and the device-to-device copy of the accumulator (skh_copy_accum, OptixRender.cpp:1022-1043)."""
import numpy as np
import pytest

from strelka_amd import scene as S, scenes

pytestmark = pytest.mark.gpu


def test_trace_on_device_arrays_equals_trace_on_host_arrays():
    import torch
    from strelka_amd import capi
    sc = scenes.kitchen_standin(seed=3, n_meshes=6, n_instances=30, tri_lo=50, tri_hi=800)
    rays = scenes.random_rays(20000, 5, -4.0, 4.0)
    ctx = capi.Context(0)
    ctx.set_scene(sc.arrays())
    for mode in (0, 1):
        want = ctx.trace(rays, mode)
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
        d_hits = torch.zeros(len(rays) * S.HIT.itemsize, dtype=torch.uint8, device="cuda")
        ctx.trace_device(d_rays.data_ptr(), len(rays), mode, d_hits.data_ptr(), repeat=2)
        ctx.synchronize()
        got = d_hits.cpu().numpy().view(S.HIT)
        assert (got.view(np.uint8) == want.view(np.uint8)).all(), "mode %d" % mode
    assert ctx.stream()  # a hipStream_t the caller may order its own work against
    ctx.close()


def test_device_info_describes_the_gpu_the_roofs_are_priced_on():
    from strelka_amd import capi
    ctx = capi.Context(0)
    info = ctx.device_info()
    ctx.close()
    assert info["wavefront_size"] == 64 and info["simds_per_cu"] == 4
    assert info["compute_units"] >= 1 and info["clock_khz"] > 100000 and info["total_memory_bytes"] > (1 << 30)
    assert "gfx950" in info["name"] or info["name"]  # (the arch string where the runtime reports it, a product name otherwise)


def test_copy_accum_is_the_accumulator():
    import torch
    from strelka_amd import capi
    sc = scenes.cornell_box()
    W = H = 64
    ctx = capi.Context(0)
    ctx.set_scene(sc.arrays())
    ctx.resize(W, H)
    p = S.frame_params(sc.getCamera(), W, H, subframe_index=0, samples_this_launch=1, spp_total=4, max_depth=3)
    ctx.render_subframes(p, 4, None)
    want = ctx.read_accum()
    d = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    ctx.copy_accum(d.data_ptr())
    ctx.synchronize()
    ctx.close()
    assert (d.cpu().numpy().reshape(H, W, 4) == want.reshape(H, W, 4)).all()


def test_build_info_reports_the_reinsertion_pass():
    """skh_get_build_info: what the last skh_build_accel did to the triangle hierarchy -- rounds, moves, the sum of the internal nodes' box areas
    before and after (the pass must lower it), its time inside ms_build; with the pass off, or on the radix-tree builder, the record says so."""
    from strelka_amd import capi, scenes

    sc = scenes.kitchen_standin(seed=5, n_meshes=12, n_instances=120, tri_lo=100, tri_hi=3000)
    arr = sc.arrays()
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    b = ctx.build_info()
    assert b["triangles"] > 10000 and b["nodes"] > 1000
    assert 1 <= b["reinsert_rounds"] <= 8 and b["reinsert_moves"] > 100 and b["reinsert_min_size"] == 1
    assert 0.5 * b["cost_before"] < b["cost_after"] < 0.99 * b["cost_before"]
    assert 0.0 < b["ms_reinsert"] < b["ms_build"]
    ctx.set_option("reinsert_rounds", 0)
    ctx.set_scene(arr)
    b0 = ctx.build_info()
    assert b0["reinsert_rounds"] == 0 and b0["reinsert_moves"] == 0 and b0["triangles"] == b["triangles"]
    ctx.set_option("reinsert_rounds", 8)
    ctx.set_option("build_quality", 0)  # the Karras radix tree has no per-group parent chain: no reinsertion
    ctx.set_scene(arr)
    assert ctx.build_info()["reinsert_rounds"] == 0
    for name, bad in (("reinsert_rounds", 65), ("reinsert_curve_rounds", -1), ("reinsert_min_size", -3)):
        with pytest.raises(capi.SkhError):
            ctx.set_option(name, bad)
    ctx.close()


# skh_set_option: every name with its inclusive range (None = no bound on that side), the value a fresh context holds, and whether a hierarchy depends on it
# (setting it costs skh_update_accel its in-place path).  Typed from the setter's code; curve_segnode / curve_strand_major accept 1 only in a library built
# with segment nodes.
OPTIONS = [
    # name, lo, hi, default, rebuild
    ("timing", None, None, 0, False), ("count_traversal", None, None, 0, False),
    ("fetch_min_closest", 1, 64, 32, False), ("fetch_min_shadow", 1, 64, 48, False), ("fetch_min_closest_small", 1, 64, 48, False), ("curve_min", 1, 64, 48, False),
    ("leaf_min", 0, 64, 16, False), ("node_break_closest", 0, 64, 32, False), ("node_break_shadow", 0, 64, 28, False), ("speculate", 0, 64, 8, False),
    ("tlas_open", 0, 64, 1, True), ("subframe_batch", 0, 64, 0, False), ("small_waves_first", 0, 64, 0, False), ("small_waves_last", 0, 64, 0, False),
    ("small_waves_closest", 0, 64, 0, False), ("small_waves_shadow", 0, 64, 0, False), ("reinsert_rounds", 0, 64, 8, True), ("reinsert_curve_rounds", 0, 64, 4, True),
    ("compact_hits", 0, 1, 1, True), ("merge_light_proxies", 0, 1, 0, True), ("curve_merge", 0, 1, 1, True), ("curve_segnode", 0, 1, 0, True),
    ("curve_strand_major", 0, 1, 0, True), ("env_nee", 0, 1, 1, False), ("speculate_async", 0, 1, 1, False), ("leaf_lines", 0, 1, 0, True),
    ("direct_records", -1, 1, -1, True), ("fetch_chunk", -1, 4096, -1, False), ("overlap", 0, 2, 1, False), ("tlas_build", 0, 2, 1, True),
    ("tail_split", -1, 2, 1, False), ("curve_leaf", 1, 4, 1, True), ("curve_split", 1, 8, 4, True), ("leaf_max_tris", 1, 8, 2, True),
    ("split_pairs", 0, 1000, 0, True), ("bake_world", 0, 4, 4, True), ("bake_budget_mtris", 0, 100, 64, True), ("bake_small_tris", 0, 1 << 20, 64, True),
    ("speculate_grow", 2, 64, 2, False), ("morton_bits", 4, 21, 10, True), ("reinsert_min_size", 0, 1 << 24, 0, True), ("ploc_top", 0, None, 0, True),
    ("waves_per_cu", 1, 32, 28, False), ("waves_per_cu_shadow", 1, 32, 28, False), ("waves_per_cu_world", 1, 32, 32, False),
    ("waves_per_cu_shadow_world", 1, 32, 32, False),
    ("tight_instance_boxes", None, None, 1, True), ("world_kernel", None, None, 1, False), ("build_quality", None, None, 1, True),
]


def _small_kitchen():
    return scenes.kitchen_standin(seed=7, n_meshes=12, n_instances=60, tri_lo=100, tri_hi=1500)


def test_option_ranges_are_inclusive_and_unknown_names_are_refused():
    """Every bounded option takes both ends of its range and refuses the values next to them, on a context without a frame and without a scene."""
    from strelka_amd import capi
    ctx = capi.Context(0)
    L, h = ctx.lib, ctx.h
    OK, INVALID = 0, 3  # SKH_OK, SKH_INVALID_ARGUMENT

    def put(name, value):
        return L.skh_set_option(h, name.encode(), int(value))

    for name, lo, hi, default, _ in OPTIONS:
        segnode = name in ("curve_segnode", "curve_strand_major")
        if lo is not None:
            assert put(name, lo) == OK, (name, lo)
            assert put(name, lo - 1) == INVALID, (name, lo - 1)
        if hi is not None:
            st = put(name, hi)
            assert st == OK or (segnode and st == INVALID), (name, hi)  # (value 1: only a library built with segment nodes takes it)
            assert put(name, hi + 1) == INVALID, (name, hi + 1)
        if lo is None and hi is None:  # any value, read as value != 0
            for v in (-(1 << 40), -1, 0, 1, 1 << 40):
                assert put(name, v) == OK, (name, v)
        if name == "ploc_top":
            assert put(name, (1 << 31) - 1) == OK
        assert put(name, default) == OK, (name, default)
    assert put("no_such_option", 1) == INVALID
    assert "no_such_option" in L.skh_last_error(h).decode()
    ctx.close()


def test_only_the_options_a_hierarchy_depends_on_cost_a_rebuild():
    """skh_update_accel's contract (include/strelka_hip.h): an option the build reads invalidates the hierarchy, every other one leaves the in-place path open.
    Each option is set to the value it already has; build_info().refit then says which path the update took (2 in place, 0 a build)."""
    from strelka_amd import capi
    ctx = capi.Context(0)
    ctx.set_scene(_small_kitchen().arrays())
    ctx.update_accel(None)
    assert ctx.build_info()["refit"] == 2
    for name, _, _, default, rebuild in OPTIONS:
        if name == "tlas_open":  # (its value blocks the update by itself)
            continue
        ctx.set_option(name, default)
        ctx.update_accel(None)
        assert ctx.build_info()["refit"] == (0 if rebuild else 2), name
    ctx.close()


def test_build_render_update_destroy_cycles_leave_no_device_memory_behind():
    """Ten cycles of create / set scene / build / one sub-frame / update / destroy over both TLAS builders, the by-line leaf layout and a curve scene may not
    cost more device memory than one default-kitchen hierarchy's nodes (64 bytes each): a cycle that lost any per-primitive buffer would exceed that ten times
    over, the allocator's granularity does not."""
    import torch
    from strelka_amd import capi
    kitchen, hair = _small_kitchen(), scenes.hair_standin(seed=5, n_strands=1500, n_cp=8)
    cases = [(kitchen, {}), (kitchen, {"bake_world": 0, "tlas_build": 1}), (kitchen, {"bake_world": 0, "tlas_build": 0}), (kitchen, {"leaf_lines": 1}), (hair, {})]
    arrays = [(sc.arrays(), sc.getCamera(), opts) for sc, opts in cases]
    W = H = 64

    def cycle():
        nodes = None
        for arr, cam, opts in arrays:
            ctx = capi.Context(0)
            for k, v in opts.items():
                ctx.set_option(k, v)
            ctx.set_scene(arr)
            if nodes is None:
                nodes = ctx.build_info()["nodes"]
            ctx.resize(W, H)
            ctx.render_subframe(S.frame_params(cam, W, H, subframe_index=0, samples_this_launch=1, spp_total=1, max_depth=3))
            ctx.update_accel(None)
            ctx.synchronize()
            ctx.close()
        return nodes

    for _ in range(2):
        nodes = cycle()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(10):
        cycle()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    print("free before %d after %d, allowance %d" % (before, after, nodes * 64))
    assert nodes > 1000
    assert after >= before - nodes * 64
