"""The GPU builders held to every primitive on tied boxes and tail counts ("Every primitive is in the hierarchy"; tests/buildref.py).

Every test builds one scene under one set of options and calls the roll: each ray of tests/buildref.py must come back from Context.trace(rays, 0) with exactly
the (instance, primitive) the float64 reference names (the smaller key where triangles coincide), the whole record bit-equal to the checker's trace of the same
scene and bake mode (whose first 4000 rays also equal its own brute-force loop), t, u and v inside the bars tests/hitref.py derives for an interior hit at that
scale (barycentric_error with L / altitude of the triangle, C_ISECT U L along the ray; the rays are perpendicular: cos = 1), every any-hit twin occluded, every ray
aimed at a degenerate triangle a miss, and build_info()["triangles"] the number of triangles handed in.  hitref's bars are for triangles: on the strand the
(instance, segment) comes from tests/curveref.py's float64 entry and t, u, v rest on the checker's bits.  Rays the float64 brute force leaves out (none today; at
most 2 % by tests/test_build_edges_cpu.py) are still compared with the checker bit for bit.

What the scenes are for.  Counts on a kernel's tail (buildref.TAIL_COUNTS: the 64-lane wave, SKH_PLOC_BLOCK and SKH_LEAF_CHUNK 256, the 4096-key blocks of the
radix sort and the scan, tlas_build 2's 8192, trees of one leaf), as one mesh, as n meshes of one triangle under three bake modes, and as rows of n instances
under the three top-level builders.  Tied boxes -- a straight strip of unit quads, n triangles that share one box, a row of equal instances, a straight strand:
under `the lowest index wins` every cluster of such a run names its LEFT neighbour in k_ploc_nn and one pair merges per round; a build that gives up with more
clusters than groups would keep one cluster per group in k_ploc_roots and lose the rest (docs/LOG.md "Tied boxes": what the previous builder lost, measured).
lbvh_ploc's switch to the paired tie rule and its last-resort rounds are what these tests hold; the last-resort rounds alone are held by
test_clusters_paired_by_position, through a build whose cost search stops after one round.

Termination on tied inputs, read from the code.  lbvh_ploc: the cost search runs at most SKH_PLOC_MAX_ROUNDS (4096) rounds, breaks ties the paired way once two
rounds in a row have each done less than a sixteenth of the merges still to do, and leaves its loop on a round without a merge; the last-resort rounds that
follow pair clusters i, i + 1 of a group by position, a run of L clusters keeps at most L / 2 + 1, the loop ends after two rounds in a row without a merge or 128
rounds, and a count that still differs from the number of non-empty groups is an error, not a tree.  k_karras: delta_keys breaks equal keys by index
(64 + clz(i ^ j)), so the keys are distinct, every search loop of the kernel is a doubling or a halving over at most n positions and ends at the first
out-of-range index (-1 is never greater than dmin >= -1); n equal keys give the balanced tree of the index bits.  The reinsertion's refit walks one level per
launch, at most n launches, reads the next level's count after every sixteenth level and after the last (soup(8) and soup(9) are trees of fewer than sixteen
levels) and fails the build rather than spin; its counter ring (SKH_RI_MAX_LEVELS) wraps and zeroes a counter before reuse, so a tree deeper than the ring costs
launches, not correctness.  k_collapse runs once per level of the binary tree with a host-side count, at most n levels.  Nothing loops on a device-side
condition."""
import functools

import numpy as np
import pytest

from tests import buildref as B
from tests import hitref

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def contexts():
    """one context per set of options, reused by every scene built under it"""
    from strelka_amd import build, capi

    build.build()
    made = {}

    def get(**options):
        key = tuple(sorted(options.items()))
        if key not in made:
            made[key] = capi.Context(0)
            for k, v in options.items():
                made[key].set_option(k, v)
        return made[key]

    yield get
    for c in made.values():
        c.close()


@functools.lru_cache(maxsize=None)
def oracle(scene, bake):
    """the checker's answers for a scene under a bake mode, once: closest hits, any-hit, the degenerate triangles' rays; its hierarchy against its own brute force"""
    from tests import orklib

    case, arr, ref, keep = B.cached(*scene)
    o = orklib.new_context()
    o.set_bake(bake)
    o.set_scene(arr)
    want = o.trace(case.rays, 0)
    assert np.array_equal(o.trace(case.rays[:4000], 0, brute=True), want[:4000])
    return want, o.trace(case.rays, 1), (o.trace(case.miss, 0), o.trace(case.miss, 1)) if len(case.miss) else None


def records_equal(a, b):
    return a.tobytes() == b.tobytes()


def call_the_roll(ctx, scene, bake, built=False):
    """builds `scene` in ctx (built: it is there already -- a refit or an update put it there) and checks everything the module docstring lists"""
    case, arr, ref, keep = B.cached(*scene)
    if not built:
        ctx.set_scene(arr)
        assert ctx.build_info()["triangles"] == case.triangles, (case.name, ctx.build_info()["triangles"], case.triangles)
    want, want_any, want_miss = oracle(scene, bake)
    got = ctx.trace(case.rays, 0)
    keep = np.ones(len(case.rays), bool) if keep is None else keep
    wrong = keep & ((got["instance_id"] != ref["inst"]) | (got["prim_id"] != ref["prim"]))
    missing = len(np.unique((case.inst * (1 << 32) + case.prim)[wrong]))
    print("%s: %d rays, %d left out by the brute force, %d wrong, %d primitives do not answer" % (case.name, len(case.rays), int((~keep).sum()), int(wrong.sum()), missing))
    assert not wrong.any(), "%s: %d of %d primitives do not answer their ray (first rays: %s -> %s)" % (case.name, missing, len(np.unique(case.inst * (1 << 32) + case.prim)),
                                                                                                     np.nonzero(wrong)[0][:4], got[wrong][:4])
    assert records_equal(got, want), "%s: %d records differ from the checker's" % (case.name, int((got != want).sum()))
    if case.strand is None:
        g = keep
        t_bar = hitref.C_ISECT * hitref.U * ref["L"]
        b_bar = hitref.barycentric_error(ref["L"] / ref["alt"], 1.0)
        et, eu, ev = np.abs(got["t"] - ref["t"]), np.abs(got["u"] - ref["u"]), np.abs(got["v"] - ref["v"])
        print("   t, u, v as multiples of their bars: %.2f %.2f %.2f" % ((et / t_bar)[g].max(), (eu / b_bar)[g].max(), (ev / b_bar)[g].max()))
        assert (et <= t_bar)[g].all() and (eu <= b_bar)[g].all() and (ev <= b_bar)[g].all(), case.name
    got_any = ctx.trace(case.rays, 1)
    assert (got_any["t"] >= 0).all(), "%s: %d any-hit twins are not occluded" % (case.name, int((got_any["t"] < 0).sum()))
    assert np.array_equal(got_any["t"].view(np.uint32), want_any["t"].view(np.uint32)), case.name
    if len(case.miss):
        m0, m1 = ctx.trace(case.miss, 0), ctx.trace(case.miss, 1)
        assert (m0["instance_id"] == MISS).all() and (m1["t"] < 0).all(), "%s: a degenerate triangle was hit" % case.name
        assert records_equal(m0, want_miss[0]) and np.array_equal(m1["t"].view(np.uint32), want_miss[1]["t"].view(np.uint32))


def ids(x):
    return "-".join(str(v) for v in x) if isinstance(x, tuple) else "_".join("%s%s" % kv for kv in x.items()) or "defaults" if isinstance(x, dict) else str(x)


TAIL_OPTIONS = [{}, {"build_quality": 0}, {"leaf_max_tris": 1}, {"leaf_max_tris": 4, "leaf_lines": 1}, {"reinsert_rounds": 0}]


@pytest.mark.parametrize("scene", B.TAIL_SCENES, ids=ids)
@pytest.mark.parametrize("options", TAIL_OPTIONS, ids=ids)
def test_tail_counts_one_mesh(contexts, options, scene):
    call_the_roll(contexts(**options), scene, 4)


@pytest.mark.parametrize("scene", B.GROUP_SCENES, ids=ids)
@pytest.mark.parametrize("bake", [3, 0, 1])
def test_tail_counts_as_groups_of_one_triangle(contexts, bake, scene):
    """bake_world 3: one world-space group built from n source groups; 0: n one-leaf trees under a top level; 1: every single-user mesh baked"""
    call_the_roll(contexts(bake_world=bake), scene, bake)


@pytest.mark.parametrize("bake", [3, 0])
def test_group_bits_squeeze_the_morton_bits(contexts, bake):
    """4097 groups take 13 bits of the key: morton_bits 21 is cut to 17 (lbvh_sort: min(morton_bits, (64 - group bits) / 3))"""
    call_the_roll(contexts(bake_world=bake, morton_bits=21), ("soup_groups", 4097), bake)


@pytest.mark.parametrize("scene", B.TOP_SCENES, ids=ids)
@pytest.mark.parametrize("tight", [0, 1])
@pytest.mark.parametrize("tlas_build", [0, 1, 2])
def test_top_level_over_rows_of_instances(contexts, tlas_build, tight, scene):
    """a row of equal, equally spaced instances (tied boxes for the top level's 96-neighbour search: 16386 of them were more than 4096 rounds could chain) and its
    jittered-lattice twin, under the host sweep, the GPU builder, and the switch between them at 8192 leaves"""
    call_the_roll(contexts(bake_world=0, tlas_build=tlas_build, tight_instance_boxes=tight), scene, 0)


BUILDERS = [{}, {"build_quality": 0}, {"ploc_top": 4096}]


@pytest.mark.parametrize("scene", B.TIED_SCENES, ids=ids)
@pytest.mark.parametrize("options", BUILDERS, ids=ids)
def test_tied_geometry(contexts, options, scene):
    """the strip, and n triangles in one box, as the only mesh and as one mesh among soups (its neighbours in key order are then other groups), under PLOC, the
    radix tree, and PLOC with the wide search for the last 4096 clusters"""
    call_the_roll(contexts(**options), scene, 4)


@pytest.mark.parametrize("curve_split", [1, 4])
def test_long_straight_strand(contexts, curve_split):
    """4099 segments of one straight strand: the curve builder's sub-segment boxes tie along the axis (search radius 8)"""
    call_the_roll(contexts(curve_split=curve_split), ("long_strand", 4099), 4)


def test_strip_after_a_refit_that_breaks_the_ties(contexts):
    """skh_refit_accel keeps the topology the tied strip was built with; the displaced strip's roll call must still be answered by every triangle"""
    ctx = contexts()
    call_the_roll(ctx, ("strip", 32770), 4)
    ctx.set_geometry(B.cached("strip_waved", 32770)[1])
    ctx.refit_accel()
    assert ctx.build_info()["refit"] == 1
    call_the_roll(ctx, ("strip_waved", 32770), 4, built=True)


def test_row_after_an_update_that_changes_its_spacing(contexts):
    """skh_update_accel under new transforms that keep the row and stretch it by half"""
    ctx = contexts(bake_world=0)
    call_the_roll(ctx, ("row", 8193), 0)
    ctx.update_accel(B.cached("row_spaced", 8193)[1]["instances"])
    assert ctx.build_info()["refit"] == 2
    call_the_roll(ctx, ("row_spaced", 8193), 0, built=True)


def test_clusters_paired_by_position(tmp_path, contexts):
    """A build with -DSKH_PLOC_MAX_ROUNDS=1: the cost search runs one round and everything else is merged by lbvh_ploc's last-resort rounds (k_ploc_nn_adjacent,
    alternating parity) -- the path no input reaches in the shipped build.  The same roll call, on the tied families, a soup, n groups of one triangle (no
    group may pair with its neighbour group), a mesh among soups, the 16386-instance row's top level and the strand."""
    import os
    import subprocess
    import sys

    from strelka_amd import build

    lib = build.build_variant(str(tmp_path / "libstrelka_hip_oneround.so"), ["SKH_PLOC_MAX_ROUNDS=1"])
    code = r'''
import os, sys
sys.path.insert(0, os.environ["SKH_ROOT"])
from strelka_amd import capi
from tests.test_gpu_build_edges import call_the_roll
for scene, options in [(("soup", 4097), {}), (("soup_decorated", 4065, 16), {}), (("soup_groups", 257), {"bake_world": 3}), (("strip", 32770), {}), (("box_twins", 8194), {}),
                       (("strip_in_soup", 32770), {}), (("box_twins_in_soup", 4097), {}), (("row", 16386), {"bake_world": 0, "tlas_build": 1}), (("long_strand", 4099), {})]:
    ctx = capi.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    call_the_roll(ctx, scene, options.get("bake_world", 4))
    ctx.close()
print("PAIRED-BY-POSITION-OK")
'''
    env = dict(os.environ, SKH_LIB=lib, SKH_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "PAIRED-BY-POSITION-OK" in out.stdout, out.stdout + out.stderr
