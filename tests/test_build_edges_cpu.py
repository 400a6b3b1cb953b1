"""tests/buildref.py held to itself on the CPU: the generators' invariants, the float64 reference's two conditions on every scene tests/test_gpu_build_edges.py builds,
the checker's hierarchy answering the same roll call, and the round counts of the builder's cluster selection under the old and the new tie rule."""
import numpy as np
import pytest

from tests import buildref as B


def _boxes(case):
    pos, tris = case.meshes[0]
    P = np.asarray(pos, np.float32)[tris]
    return P.min(axis=1), P.max(axis=1)


@pytest.mark.parametrize("n", [1, 2, 9, 257, 4097])
def test_soup_triangles_sit_inside_their_cells(n):
    case = B.soup(n)
    P = np.asarray(case.meshes[0][0], np.float64).reshape(n, 3, 3)
    cell = np.floor(P.mean(axis=1))
    assert len(np.unique(cell, axis=0)) == n  # one triangle per cell
    assert (np.abs(P - (cell + 0.5)[:, None, :]).max(axis=(1, 2)) <= 0.3 + 1e-6).all()  # well inside it
    edges = np.linalg.norm(P - np.roll(P, 1, axis=1), axis=2)
    assert edges.max() <= 0.4 and edges.min() > 0.3
    o = np.asarray(case.rays["origin"], np.float64)
    assert (np.abs(o - (cell + 0.5)).max(axis=1) < 0.3).all() and len(case.rays) == n


def test_strip_coordinates_are_small_integers_and_its_boxes_tie():
    case = B.strip(32770)
    pos, tris = case.meshes[0]
    assert pos.dtype == np.float32 and np.array_equal(pos, np.round(pos)) and pos.max() == 16385 and len(tris) == 32770
    lo, hi = _boxes(case)
    assert np.array_equal(lo[0::2], lo[1::2]) and np.array_equal(hi[0::2], hi[1::2])  # the two triangles of a quad share its box
    assert np.array_equal(hi - lo, np.tile(np.float32([1, 1, 0]), (32770, 1)))


@pytest.mark.parametrize("n", [4097, 8194])
def test_box_twins_share_one_box_bit_for_bit_and_nothing_but_the_diagonal(n):
    case = B.box_twins(n)
    lo, hi = _boxes(case)
    assert np.array_equal(lo.view(np.uint32), np.zeros((n, 3), np.uint32)) and np.array_equal(hi.view(np.uint32), np.tile(np.float32(1).view(np.uint32), (n, 3)))
    P = np.asarray(case.meshes[0][0], np.float64).reshape(n, 3, 3)
    assert np.array_equal(P[:, 0], np.zeros((n, 3))) and np.array_equal(P[:, 1], np.ones((n, 3)))
    third = P[:, 2]
    assert len(np.unique(third, axis=0)) == n and (third > 0).all() and (third < 1).all()
    # the third vertices go round the diagonal once, every step in the same sense: the half planes through the diagonal are pairwise distinct
    axis = np.ones(3) / np.sqrt(3.0)
    r = third - 0.5 - ((third - 0.5) @ axis)[:, None] * axis
    turn = np.cross(r, np.roll(r, -1, axis=0)) @ axis
    assert (turn > 0).all() and np.abs(np.linalg.norm(r, axis=1) - B.TWIN_RADIUS).max() < 1e-6
    assert len(case.rays) == 3 * n and case.h.max() < 0.2 * 2e-4 * 8194 / n


def test_row_and_strand_are_evenly_spaced():
    case = B.row_of_instances(257)
    c = np.stack([np.asarray(m)[:, 3] for _, _, m in case.instances])
    assert np.array_equal(c, np.stack([np.arange(257), np.zeros(257), np.zeros(257)], 1)) and len(case.meshes[0][1]) == 12
    s = B.long_strand(4099)
    pts, radius = s.strand
    assert np.array_equal(np.diff(pts, axis=0), np.tile(np.float32([1, 0, 0]), (4101, 1))) and len(s.rays) == 4099 and radius == B.STRAND_RADIUS


def test_decorations_keep_the_roll_call_and_name_the_smaller_key():
    base = B.soup(300)
    case = B.with_duplicates(B.with_degenerates(base, 24), 24)
    pos, tris = case.meshes[0]
    assert case.triangles == 348 and len(case.miss) == 24 and len(case.alt) == 24
    P = np.asarray(pos, np.float64)[tris]
    area = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    assert (area == 0).sum() >= 24  # exactly degenerate in float32: two equal vertices, or three that differ in one coordinate (a repeat may have copied one)
    for r, keys in case.alt.items():
        prims = [p for _, p in keys]
        assert case.prim[r] == min(prims) and len(prims) >= 2
        assert all(np.array_equal(tris[p], tris[prims[0]]) for p in prims)
    # the real triangles are the base's, in the base's order
    real = area > 0
    first_of = np.unique(tris[real], axis=0, return_index=True)[1]
    assert len(first_of) == 300
    g = B.as_groups(case)
    assert len(g.meshes) == 348 and np.array_equal(g.inst, case.prim) and (g.prim == 0).all() and g.triangles == 348


@pytest.mark.parametrize("scene", B.GPU_SCENES, ids=lambda s: "-".join(str(x) for x in s))
def test_reference_conditions_hold_on_every_scene_the_gpu_test_builds(scene):
    """At most 2 % of a scene's rays fail the brute-force margin and every primitive keeps a ray (scenes of up to BRUTE_MAX triangles: the others are the same
    constructions at a size the brute force is not run at); the roll call's own hit is interior (every weight >= 0.2) and inside the interval on every scene."""
    case, arr, ref, keep = B.cached(*scene)
    called = len(np.unique(case.inst * (1 << 32) + case.prim))
    row = case.name.startswith("row_of_instances")
    if case.strand is None and not row:  # every real triangle is called, once under the smallest of its keys
        assert called == case.triangles - _degenerate(case) - _repeats(case)
    elif row:
        assert called == 2 * len(case.instances)  # a row: the two triangles of every instance's top face
    if case.strand is not None:
        assert np.array_equal(ref["inst"], case.inst) and np.array_equal(ref["prim"], case.prim)
        assert np.abs(ref["t"] - 3 * B.STRAND_RADIUS).max() < 1e-7 and np.abs(ref["u"] - 0.5).max() < 1e-6
        return
    w = np.minimum(np.minimum(ref["u"], ref["v"]), 1 - ref["u"] - ref["v"])
    assert (w >= 0.2 - 1e-6).all() and (np.abs(ref["t"] - case.h) <= 1e-3 * case.h + 4 * B.ULP * ref["L"]).all()  # (the origin is rounded to float32)
    if keep is None:
        return
    excluded, uncovered = B.check_cover(case, keep)
    assert excluded <= B.MAX_EXCLUDED and uncovered == 0, (excluded, uncovered)


def _degenerate(case):
    n = 0
    for pos, tris in case.meshes:
        P = np.asarray(pos, np.float64)[np.asarray(tris)]
        n += int((np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1) == 0).sum())
    return n


def _repeats(case):
    """repeated real triangles (with_duplicates; after as_groups they are meshes of their own)"""
    return len({k for keys in case.alt.values() for k in keys}) - len(case.alt)


@pytest.mark.parametrize("scene", [("soup_decorated", 225, 16), ("soup_groups_decorated", 225, 16), ("strip_decorated", 520, 16), ("box_twins", 4097), ("row_jittered", 257),
                                   ("strip_waved", 8000), ("long_strand", 300)], ids=lambda s: "-".join(str(x) for x in s))
def test_the_checker_answers_the_roll_call(ork, scene):
    """The checker's SAH hierarchy and its brute-force loop report the reference's (instance, primitive) on every kept ray, the smaller key of coincident triangles,
    nothing on the degenerate triangles' rays, and occlusion for every any-hit twin: the reference and the oracle the GPU test compares with agree with each other."""
    from tests import orklib

    case, arr, ref, keep = B.cached(*scene)
    o = orklib.new_context()
    o.set_bake(0)
    o.set_scene(arr)
    keep = np.ones(len(case.rays), bool) if keep is None else keep
    for brute in (False, True):
        h = o.trace(case.rays, 0, brute=brute)
        assert np.array_equal(h["instance_id"][keep], ref["inst"][keep]) and np.array_equal(h["prim_id"][keep], ref["prim"][keep])
    assert (o.trace(case.rays, 1)["t"] >= 0).all()
    if len(case.miss):
        assert (o.trace(case.miss, 0)["instance_id"] == 0xFFFFFFFF).all() and (o.trace(case.miss, 1)["t"] < 0).all()


def test_the_incremental_round_count_equals_the_plain_one():
    for case, radius in ((B.soup(700), 12), (B.strip(700), 12), (B.box_twins(300), 12), (B.row_of_instances(300), 8)):
        lo, hi = B.boxes_of(case)
        k = B.morton_order(lo, hi)
        assert B.ploc_rounds(lo[k], hi[k], radius, "lowest") == B.ploc_rounds(lo[k], hi[k], radius, "lowest", incremental=False)


# (input, size, search radius, rounds of the old rule that are run).  96 is the top level's radius: a chained round costs numpy 7 ms there, so 256 rounds are run
# in place of 4096 -- what they leave shows the rate, fewer than three merges a round
TIED = [("strip", 32770, 12, 4096), ("box_twins", 8194, 12, 4096), ("row", 16386, 8, 4096), ("row", 16386, 96, 256)]


@pytest.mark.parametrize("name,n,radius,cap", TIED)
def test_tied_inputs_chain_under_the_old_rule_and_pair_off_under_the_new(name, n, radius, cap):
    """`lowest index wins` merges fewer than three pairs a round on tied boxes and is out of rounds (4096) with thousands of clusters left; the new rule -- the
    paired tie break once two rounds in a row have stalled, as lbvh_ploc applies it -- brings the same input down to one cluster in no more than twice the rounds
    a soup of the same size takes under the OLD rule (the reference for "normal": 2.4 to 3.1 log2 n), and leaves the soup's count where it was.  The counts are
    quoted in docs/LOG.md."""
    lo, hi = B.boxes_of(B.FAMILIES[name](n))
    k = B.morton_order(lo, hi)
    lo, hi = lo[k], hi[k]
    rounds_old, left_old = B.ploc_rounds(lo, hi, radius, "lowest", cap=cap)
    assert rounds_old == cap and left_old > (1000 if cap == 4096 else n - 3 * cap), (rounds_old, left_old)
    slo, shi = B.boxes_of(B.soup(n))
    k = B.morton_order(slo, shi)
    normal, left = B.ploc_rounds(slo[k], shi[k], radius, "lowest")
    assert left == 1
    allowed = 2 * normal
    rounds_new, left_new = B.ploc_rounds(lo, hi, radius, "adaptive")
    soup_new, soup_left = B.ploc_rounds(slo[k], shi[k], radius, "adaptive")
    rounds_pure, left_pure = B.ploc_rounds(lo, hi, radius, "paired")
    print("%s(%d), radius %d: old rule %d rounds, %d clusters left; new rule %d rounds (paired throughout: %d); soup old %d, new %d; log2 n %.1f"
          % (name, n, radius, rounds_old, left_old, rounds_new, rounds_pure, normal, soup_new, np.log2(n)))
    assert left_pure == 1 and rounds_pure <= allowed, (rounds_pure, allowed)
    assert left_new == 1 and rounds_new <= allowed, (rounds_new, allowed)
    assert soup_left == 1 and soup_new <= allowed, (soup_new, allowed)
