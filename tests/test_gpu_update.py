"""skh_update_accel (-m gpu): every level of the acceleration structure updated in place after edited instance transforms, vertices and curve control
points -- the baked world-space triangles, the object-space BLASes, the instance records and the TLAS (refitted level by level on the device).

Hit records do not depend on the hierarchy, so the bar everywhere is the oracle of the EDITED scene, bit for bit: closest-hit and any-hit records and
rendered images equal, no tolerance.  build_info()["refit"] says what happened: 2 = updated in place, 0 = the documented fallback to a full build.
"""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests.test_gpu_parity import _image_equal, assert_hits_equal, camera_rays, small_kitchen

pytestmark = pytest.mark.gpu

HALF_ROOM = np.array([2.5, 1.0, 1.5])  # half of the kitchen's 10 x 4 x 6 room


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def _moves(rs, n, reach):
    """n rigid-ish moves (4x4): a rotation about a random axis, a non-uniform scale in [0.6, 1.4], a translation up to `reach` per axis"""
    out = []
    for _ in range(n):
        M = np.eye(4)
        M[:3, :3] = _rotation(rs.normal(size=3), rs.uniform(-math.pi, math.pi)) @ np.diag(rs.uniform(0.6, 1.4, 3))
        M[:3, 3] = rs.uniform(-1.0, 1.0, 3) * reach
        out.append(M)
    return out


def _moved(instances, idx, moves):
    """the instance table with instance idx[k] carried by moves[k] (applied in world space, in float64, rounded once)"""
    inst = instances.copy()
    for i, M in zip(idx, moves):
        X = np.eye(4)
        X[:3, :] = inst["transform"][i].reshape(3, 4)
        inst["transform"][i] = (M @ X)[:3, :].reshape(-1).astype(np.float32)
    return inst


def _with(arr, **kw):
    b = dict(arr)
    b.update(kw)
    return b


def _oracle(arr, bake=None):
    from tests import orklib

    o = orklib.new_context()
    if bake is not None:
        o.set_bake(bake)
    o.set_scene(arr)
    return o


def _kitchen_rays(sc):
    rays = np.concatenate([camera_rays(sc, 64, 64, 12000, 3), scenes.random_rays(12000, 4, -3.5, 3.5)])
    rays["origin"][12000:, 1] = np.abs(rays["origin"][12000:, 1]) * 0.8 + 0.05
    return rays


def _check_hits(ctx, o, rays, tmax=3.0):
    want = o.trace(rays, 0)
    assert_hits_equal(ctx.trace(rays, 0), want)
    r2 = rays.copy()
    r2["tmax"] = tmax
    assert np.array_equal(ctx.trace(r2, 1)["t"], o.trace(r2, 1)["t"])
    return want


def _render(r, sc, w, h, first, n, spp):
    for i in range(first, first + n):
        r.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=i, spp_total=spp, max_depth=4))


def _edited_vertices(arr, amount):
    v = arr["vertices"].copy()
    p = v["pos"].astype(np.float64)
    p += amount * np.stack([np.sin(3.1 * p[:, 1] + 0.3), np.cos(2.3 * p[:, 2]), np.sin(1.7 * p[:, 0] + 1.1)], 1)
    v["pos"] = p.astype(np.float32)
    return v


def test_update_moves_instances_of_the_baked_kitchen_in_place():
    """Default options: every mesh instance baked to world space, no top level.  One instance, a third of them, then all of them move (rotations, non-uniform
    scales, translations up to half the room): each update is in place and returns the edited scene's hit records and image; twenty updates in a row leave no drift."""
    from strelka_amd import capi

    sc = small_kitchen()
    arr = dict(sc.arrays())
    rays = _kitchen_rays(sc)
    rs = np.random.RandomState(21)
    mesh = np.nonzero(arr["instances"]["type"] == S.INSTANCE_MESH)[0]
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    assert ctx.build_info()["refit"] == 0
    flags, n_baked, _ = ctx.baked(len(arr["instances"]))
    assert flags[mesh].all()  # (the scene this test is about: no mesh instance keeps a TLAS leaf)
    cur = arr
    for sel in (mesh[5:6], mesh[::3], mesh):
        cur = _with(cur, instances=_moved(cur["instances"], sel, _moves(rs, len(sel), HALF_ROOM)))
        ctx.update_accel(cur["instances"])
        bi = ctx.build_info()
        assert bi["refit"] == 2 and bi["ms_refit"] > 0
        _check_hits(ctx, _oracle(cur), rays)
    # a render through the updated hierarchy (shading tables follow the transforms)
    o = _oracle(cur)
    o.resize(96, 64)
    ctx.resize(96, 64)
    _render(o, sc, 96, 64, 0, 3, 3)
    _render(ctx, sc, 96, 64, 0, 3, 3)
    _image_equal(ctx.read_accum(), o.read_accum())
    # twenty small updates in a row: the records of the last one are the edited scene's, nothing accumulated
    for k in range(20):
        sel = rs.choice(mesh, 8, replace=False)
        cur = _with(cur, instances=_moved(cur["instances"], sel, _moves(rs, len(sel), 0.2 * HALF_ROOM)))
        ctx.update_accel(cur["instances"])
        assert ctx.build_info()["refit"] == 2
    _check_hits(ctx, _oracle(cur), rays)
    ctx.close()


@pytest.mark.parametrize("tlas_build", [0, 1, 2])
@pytest.mark.parametrize("tight", [0, 1])
def test_update_of_a_two_level_kitchen_refits_the_tlas(tlas_build, tight):
    """bake_world 0: every instance keeps its TLAS leaf.  One update carries moved instances AND a vertex edit: the BLASes are refitted, the instance boxes
    recomputed from their new root boxes, the TLAS (host sweep, GPU PLOC, or the sweep because the scene is small) refitted level by level."""
    from strelka_amd import capi

    sc = small_kitchen()
    arr = dict(sc.arrays())
    rays = _kitchen_rays(sc)
    rs = np.random.RandomState(31 + tlas_build)
    mesh = np.nonzero(arr["instances"]["type"] == S.INSTANCE_MESH)[0]
    ctx = capi.Context(0)
    ctx.set_option("bake_world", 0)
    ctx.set_option("tlas_build", tlas_build)
    ctx.set_option("tight_instance_boxes", tight)
    ctx.set_scene(arr)
    sel = mesh[1::2]
    a2 = _with(arr, vertices=_edited_vertices(arr, 0.05), instances=_moved(arr["instances"], sel, _moves(rs, len(sel), HALF_ROOM)))
    ctx.set_geometry(a2)
    ctx.update_accel(a2["instances"])
    assert ctx.build_info()["refit"] == 2
    _check_hits(ctx, _oracle(a2, bake=0), rays)
    # then transforms alone (the BLASes stay as they are)
    a3 = _with(a2, instances=_moved(a2["instances"], mesh[::4], _moves(rs, len(mesh[::4]), HALF_ROOM)))
    ctx.update_accel(a3["instances"])
    assert ctx.build_info()["refit"] == 2
    _check_hits(ctx, _oracle(a3, bake=0), rays)
    ctx.close()


def _hair(n_prims, **kw):
    return scenes.hair_standin(seed=5, n_strands=1500, n_cp=8, n_prims=n_prims, prim_offset=0.05, **kw)


def _hair_rays(sc):
    return np.concatenate([camera_rays(sc, 64, 64, 20000, 11), scenes.random_rays(8000, 12, -2.0, 2.0)])


def _swayed(arr, amount):
    p = arr["curve_points"].astype(np.float64)
    p += amount * np.stack([np.sin(5.0 * p[:, 1] + 0.4), 0.3 * np.cos(4.0 * p[:, 0]), np.sin(3.0 * p[:, 2] + 1.0)], 1) * np.linalg.norm(p, axis=1, keepdims=True)
    return _with(arr, curve_points=p.astype(np.float32), curve_radii=(arr["curve_radii"] * np.float32(1.2)).astype(np.float32))


@pytest.mark.parametrize("case", ["two_world_entries", "one_merged_group", "two_level"])
def test_update_moves_curve_prims_with_a_control_point_edit(case):
    """Curve prims under transforms of their own move together with a control-point edit: two world-curve entries (SKH_WORLD_CURVES is 2), one merged group of four
    prims under one transform (every member gets the same new one), eight prims (beyond the table: curve BLASes under a TLAS)."""
    from strelka_amd import capi

    n_prims, kw = {"two_world_entries": (2, {}), "one_merged_group": (4, {"shared_xform": True}), "two_level": (8, {})}[case]
    sc = _hair(n_prims, **kw)
    arr = dict(sc.arrays())
    rays = _hair_rays(sc)
    rs = np.random.RandomState(41)
    curve = np.nonzero(arr["instances"]["type"] == S.INSTANCE_CURVE)[0]
    assert len(curve) == n_prims
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    moves = _moves(rs, 1, 0.3) * len(curve) if case == "one_merged_group" else _moves(rs, len(curve), 0.3)
    a2 = _swayed(arr, 0.02)
    a2["instances"] = _moved(arr["instances"], curve, moves)
    ctx.set_curves(a2)
    ctx.update_accel(a2["instances"])
    assert ctx.build_info()["refit"] == 2
    want = _check_hits(ctx, _oracle(a2), rays, tmax=4.0)
    assert np.isin(want["instance_id"], curve).mean() > 0.01
    ctx.close()


def test_update_takes_the_table_it_is_given_or_the_one_set_instances_left():
    """skh_update_accel(table) after skh_set_instances set a table of ANOTHER count: the update's table (the built count, moved) replaces it and is updated in
    place -- every record sized by that count, renders included; skh_update_accel(NULL) takes what skh_set_instances set: in place for moved transforms, the build
    for another count."""
    from strelka_amd import capi

    sc = small_kitchen()
    arr = dict(sc.arrays())
    rays = _kitchen_rays(sc)
    rs = np.random.RandomState(61)
    mesh = np.nonzero(arr["instances"]["type"] == S.INSTANCE_MESH)[0]
    longer = np.concatenate([arr["instances"], arr["instances"][mesh[3:4]]])
    longer["transform"][-1] = _moved(arr["instances"], mesh[3:4], _moves(rs, 1, HALF_ROOM))["transform"][mesh[3]]
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    w, h = 96, 64
    ctx.resize(w, h)
    # a table of one more instance, then the update with a moved table of the built count
    ctx.set_instances(longer)
    a2 = _with(arr, instances=_moved(arr["instances"], mesh[::5], _moves(rs, len(mesh[::5]), HALF_ROOM)))
    ctx.update_accel(a2["instances"])
    assert ctx.build_info()["refit"] == 2
    _check_hits_and_render(ctx, a2, sc, rays, w, h)
    # NULL: the table skh_set_instances set -- moved transforms (in place) ...
    a3 = _with(a2, instances=_moved(a2["instances"], mesh[1::5], _moves(rs, len(mesh[1::5]), HALF_ROOM)))
    ctx.set_instances(a3["instances"])
    ctx.update_accel()
    assert ctx.build_info()["refit"] == 2
    _check_hits_and_render(ctx, a3, sc, rays, w, h)
    # ... another count (the build)
    ctx.set_instances(longer)
    ctx.update_accel()
    assert ctx.build_info()["refit"] == 0
    _check_hits_and_render(ctx, _with(arr, instances=longer), sc, rays, w, h)
    ctx.close()


def _check_hits_and_render(ctx, arr, sc, rays, w, h):
    o = _oracle(arr)
    _check_hits(ctx, o, rays)
    o.resize(w, h)
    _render(o, sc, w, h, 0, 2, 2)
    _render(ctx, sc, w, h, 0, 2, 2)
    _image_equal(ctx.read_accum(), o.read_accum())


def test_update_falls_back_to_the_build_where_it_must():
    """Each edit the in-place update cannot keep gives refit == 0 and still the edited scene's records: a changed material_id, a singular transform, a transform
    that stops being singular, another index buffer, a merged curve group split by a transform, a moved world-curve entry that sat under the identity, tlas_open 8.
    (Another instance count: test_update_takes_the_table_it_is_given_or_the_one_set_instances_left.)"""
    from strelka_amd import capi

    sc = small_kitchen()
    arr = dict(sc.arrays())
    rays = _kitchen_rays(sc)
    mesh = np.nonzero(arr["instances"]["type"] == S.INSTANCE_MESH)[0]
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    inst = arr["instances"].copy()
    inst["material_id"][mesh[3]] = (inst["material_id"][mesh[3]] + 1) % len(arr["materials"])
    a2 = _with(arr, instances=inst)
    ctx.update_accel(a2["instances"])
    assert ctx.build_info()["refit"] == 0
    _check_hits(ctx, _oracle(a2), rays)
    inst = a2["instances"].copy()
    inst["transform"][mesh[4]] = 0.0  # singular: the instance drops out
    a3 = _with(a2, instances=inst)
    ctx.update_accel(a3["instances"])
    assert ctx.build_info()["refit"] == 0
    _check_hits(ctx, _oracle(a3), rays)
    # ... and back: the instance was built singular (no bake, no leaf), now it has a transform again
    a4 = _with(a3, instances=_moved(arr["instances"], mesh[5:6], _moves(np.random.RandomState(6), 1, HALF_ROOM)))
    a4["instances"]["material_id"] = a3["instances"]["material_id"]
    ctx.update_accel(a4["instances"])
    assert ctx.build_info()["refit"] == 0
    _check_hits(ctx, _oracle(a4), rays)
    # another index buffer (two triangles of mesh 0 swapped) with moved instances
    idx = a4["indices"].copy()
    o0 = int(a4["meshes"][0]["index_offset"])
    idx[o0:o0 + 3], idx[o0 + 3:o0 + 6] = a4["indices"][o0 + 3:o0 + 6].copy(), a4["indices"][o0:o0 + 3].copy()
    a5 = _with(a4, indices=idx, instances=_moved(a4["instances"], mesh[6:7], _moves(np.random.RandomState(7), 1, HALF_ROOM)))
    ctx.set_geometry(a5)
    ctx.update_accel(a5["instances"])
    assert ctx.build_info()["refit"] == 0
    _check_hits(ctx, _oracle(a5), rays)
    ctx.close()
    # tlas_open > 1: the opened leaves are BLAS subtrees
    ctx = capi.Context(0)
    ctx.set_option("bake_world", 0)
    ctx.set_option("tlas_open", 8)
    ctx.set_scene(arr)
    a6 = _with(arr, instances=_moved(arr["instances"], mesh[2:3], _moves(np.random.RandomState(3), 1, HALF_ROOM)))
    ctx.update_accel(a6["instances"])
    assert ctx.build_info()["refit"] == 0
    _check_hits(ctx, _oracle(a6, bake=0), rays)
    ctx.close()
    # curves: a merged group split by a transform; a world-curve entry under the identity that moves
    for sc, moved_prim in ((_hair(4, shared_xform=True), 0), (_hair(2, n_moved=1), 1)):
        arr = dict(sc.arrays())
        rays = _hair_rays(sc)
        curve = np.nonzero(arr["instances"]["type"] == S.INSTANCE_CURVE)[0]
        ctx = capi.Context(0)
        ctx.set_scene(arr)
        ctx.update_accel(arr["instances"])  # (nothing moved: in place)
        assert ctx.build_info()["refit"] == 2
        a2 = _with(arr, instances=_moved(arr["instances"], curve[moved_prim:moved_prim + 1], _moves(np.random.RandomState(4), 1, 0.3)))
        ctx.update_accel(a2["instances"])
        assert ctx.build_info()["refit"] == 0
        _check_hits(ctx, _oracle(a2), rays, tmax=4.0)
        ctx.close()


def test_update_drops_subframes_traced_ahead():
    """Default speculate: sub-frames 0-3, an update, sub-frames 0-3 again -- the accumulation is the oracle's frame of the MOVED scene: nothing traced ahead
    for the old transforms survives the update."""
    from strelka_amd import capi

    sc = small_kitchen()
    arr = dict(sc.arrays())
    mesh = np.nonzero(arr["instances"]["type"] == S.INSTANCE_MESH)[0]
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    w, h = 96, 64
    ctx.resize(w, h)
    _render(ctx, sc, w, h, 0, 4, 8)
    a2 = _with(arr, instances=_moved(arr["instances"], mesh[::2], _moves(np.random.RandomState(51), len(mesh[::2]), HALF_ROOM)))
    ctx.update_accel(a2["instances"])
    assert ctx.build_info()["refit"] == 2
    _render(ctx, sc, w, h, 0, 4, 8)
    o = _oracle(a2)
    o.resize(w, h)
    _render(o, sc, w, h, 0, 4, 8)
    _image_equal(ctx.read_accum(), o.read_accum())
    ctx.close()
