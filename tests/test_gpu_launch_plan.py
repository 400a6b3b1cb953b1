"""The render pass's launch choices ("Host side of the build"): which k_trace build a launch runs, with or without the traversal
counters; how many spans a pass opens per kernel class; that the scheduling options (overlap, tail_split, speculate) change when and where launches run and
never what they compute.  All comparisons are array_equal on the bit patterns."""
import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import cutref
from tests.test_gpu_blend import blend_of
from tests.test_gpu_cutout import make_ctx

pytestmark = pytest.mark.gpu

COUNTERS = ("launches_trace_closest", "launches_trace_shadow", "launches_shade")


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def small_hair(moved):
    # two curve sets; `moved`: the first one under a translation (the two-level curve build), else both under the identity (the world-only build with the curve block)
    return scenes.hair_standin(n_strands=400, n_prims=2, prim_offset=0.25 if moved else 0.0, n_moved=1 if moved else None)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1: count_traversal is neutral in every build of the trace kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------
MESH_BUILDS = {"world": {"tail_split": 0}, "world-split": {"tail_split": 2}}
BUILDS = [(name, opts, table) for name, opts in MESH_BUILDS.items() for table in ("none", "cutout", "blend")] + [
    ("two-level", {"bake_world": 0}, "none"), ("world-curves", {}, "none"), ("two-level-curves", {}, "none")]


@pytest.mark.parametrize("build,options,table", BUILDS, ids=["%s-%s" % (b[0], b[2]) for b in BUILDS])
def test_count_traversal_changes_no_hit_record(build, options, table):
    c = make_ctx(**options)
    if "curves" in build:
        sc = small_hair(build == "two-level-curves")
        c.set_scene(sc.arrays())
        rays = scenes.random_rays(4096, 3, -1.6, 1.6)
    else:
        sc, cut, _ = cutref.card_scene(False, "single")
        c.set_scene(sc.arrays())
        if table == "cutout":
            c.set_material_cutouts(cut)
            assert c.cutout_info()["instances"] > 0
        elif table == "blend":
            c.set_material_blend(blend_of(cut))
            assert c.blend_info()["instances"] > 0
        rays = cutref.card_rays("single", True, 4096)
    assert len(rays) == 4096
    for mode in (0, 1):
        q = cutref.shadow_version(rays) if mode == 1 else rays
        out = []
        for flag in (0, 1):
            c.set_option("count_traversal", flag)
            c.reset_stats()
            hits = c.trace(q, mode)
            out.append((hits, c.stats()["nodes_visited"]))
        (h0, n0), (h1, n1) = out
        for f in h0.dtype.names:
            assert bits_equal(h0[f], h1[f]), (mode, f)
        # The counters are per kernel build: [1] is the any-hit build's (skh_stats).  With a cutout or a blend entry in use a shadow query wants the nearest hits and
        # runs closest-hit launches, so its nodes are counted under [0]; nothing is counted under the other index either way.
        k = 0 if table != "none" else mode
        assert n0 == [0, 0] and n1[k] > 0 and n1[1 - k] == 0, (mode, n0, n1)
        assert len(np.unique(h0["t"])) > 1  # (some rays hit, some do not)
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2: the launch schedule: one span per kernel class, bounce and sample -- the cutout rounds run inside the trace spans
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_spans_per_pass():
    sc = scenes.cornell_box()
    w = h = 64
    depth, S_ = 3, 2
    c = make_ctx()
    c.set_scene(sc.arrays())
    c.resize(w, h)
    p = S.frame_params(sc.getCamera(), w, h, subframe_index=0, samples_this_launch=S_, spp_total=8, max_depth=depth)
    c.reset_stats()
    c.render_subframes(p, 1)
    st = c.stats()
    assert [st[k] for k in COUNTERS] == [S_ * depth] * 3
    # a cutout in use (the red wall, opaque everywhere): the same counts
    c.set_material_cutouts(cutref.table(3, {1: cutref.entry(opacity_scale=0.0, opacity_bias=1.0, threshold=0.5)}))
    assert c.cutout_info()["instances"] == 1
    c.reset_stats()
    c.render_subframes(p, 1)
    st = c.stats()
    assert [st[k] for k in COUNTERS] == [S_ * depth] * 3
    c.close()
    # four single-sample sub-frames traced as one pass
    c = make_ctx(subframe_batch=4)
    c.set_scene(sc.arrays())
    c.resize(w, h)
    c.reset_stats()
    c.render_subframes(S.frame_params(sc.getCamera(), w, h, subframe_index=0, samples_this_launch=1, spp_total=8, max_depth=depth), 4)
    st = c.stats()
    assert [st[k] for k in COUNTERS] == [depth] * 3
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3: scheduling options do not change the image
# ---------------------------------------------------------------------------------------------------------------------------------------------
def accum(c, sc, w, h, spp):
    c.resize(w, h)
    c.render_subframes(S.frame_params(sc.getCamera(), w, h, subframe_index=0, spp_total=spp, max_depth=4), spp)
    return c.read_accum()


@pytest.mark.parametrize("kind", ["triangles", "curves"])
def test_overlap_and_tail_split_change_no_pixel(kind):
    sc = scenes.cornell_box() if kind == "triangles" else small_hair(False)
    arr = sc.arrays()
    c = make_ctx()
    c.set_scene(arr)
    want = accum(c, sc, 64, 64, 2)
    assert np.isfinite(want).all() and (want[..., :3] > 0).any()
    for overlap in (0, 1, 2):
        for split in (0, 1, 2):
            c.set_option("overlap", overlap)
            c.set_option("tail_split", split)
            assert bits_equal(accum(c, sc, 64, 64, 2), want), (overlap, split)
    c.close()


def test_per_pass_split_changes_no_pixel():
    # 512 x 256 = 2^17 paths: the smallest pass that takes the SPLIT build under tail_split -1
    sc = scenes.cornell_box()
    c = make_ctx(tail_split=0)
    c.set_scene(sc.arrays())
    want = accum(c, sc, 512, 256, 1)
    c.set_option("tail_split", -1)
    assert bits_equal(accum(c, sc, 512, 256, 1), want)
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4: the speculative path's three kinds of pass: traced and delivered, traced only, delivered only
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_speculation_changes_no_pixel_and_discards_nothing():
    import torch

    sc = scenes.cornell_box()
    w = h = 64
    c = make_ctx()
    c.set_scene(sc.arrays())
    img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    out = {}
    for spec, asy in ((0, 0), (8, 1), (8, 0)):
        c.set_option("speculate", spec)
        c.set_option("speculate_async", asy)
        c.resize(w, h)
        c.reset_stats()
        for i in range(12):
            c.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=i, spp_total=64, max_depth=4), img.data_ptr())
        st = c.stats()
        out[(spec, asy)] = (c.read_accum(), st["speculated_discarded"], st["launches_trace_closest"])
    want, dropped, launches = out[(0, 0)]
    assert dropped == 0
    for key in ((8, 1), (8, 0)):
        assert bits_equal(out[key][0], want), key
        assert out[key][1] == 0, key
        assert out[key][2] < launches, key  # (it did trace ahead: fewer, larger passes)
    c.close()
