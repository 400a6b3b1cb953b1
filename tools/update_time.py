"""skh_update_accel against skh_build_accel (DESIGN.md section 2 "in-place updates", docs/LOG.md).  usage (GPU box): python tools/update_time.py

Cases: the kitchen stand-in baked (default options: one instance moved, every instance moved), the same kitchen with bake_world 0 (transforms only:
the TLAS is refitted, the BLASes stay), the 10^5-instance scene of tests/test_gpu_fullsize.py::test_tlas_build_on_the_gpu_scales_to_1e5_instances
(default options = baked, and bake_world 0), the hair stand-in cut into 8 prims under transforms of their own (curve BLASes under a TLAS).
Times are the library's own wall times (skh_build_info.ms_refit / ms_build), medians of a few calls; every update alternates between two tables,
so that each one moves what it says.  Last: ms_trace_closest of one 1080p sub-frame through the kitchen as built, after one instance moved and after every instance moved by up
to half the room (updated in place), and through a rebuild of the last -- what a caller gives up by not rebuilding after a large move.
Prints one JSON object."""
import json
import math
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

from strelka_amd import capi, scene as S, scenes  # noqa: E402

HALF_ROOM = np.array([2.5, 1.0, 1.5])


def moves(rs, inst, idx, reach):
    out = inst.copy()
    for i in idx:
        a = rs.normal(size=3)
        a /= np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        ang = rs.uniform(-math.pi, math.pi)
        M = np.eye(4)
        M[:3, :3] = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
        M[:3, 3] = rs.uniform(-1.0, 1.0, 3) * reach
        X = np.eye(4)
        X[:3, :] = inst["transform"][i].reshape(3, 4)
        out["transform"][i] = (M @ X)[:3, :].reshape(-1).astype(np.float32)
    return out


def measure(ctx, a, b, reps=7):
    """median ms of skh_update_accel alternating between tables a and b, median ms of skh_build_accel of b"""
    ups = []
    for k in range(reps):
        ctx.update_accel(b if k % 2 == 0 else a)
        bi = ctx.build_info()
        assert bi["refit"] == 2, bi
        ups.append(bi["ms_refit"])
    builds = []
    for k in range(3):
        ctx.build_accel()
        builds.append(ctx.stats()["ms_build"])
    return {"update_ms": float(np.median(ups)), "build_ms": float(np.median(builds)), "update_ms_all": [round(x, 3) for x in ups]}


def case(arr, idx, reach, seed, options=()):
    ctx = capi.Context(0)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.set_scene(arr)
    rs = np.random.RandomState(seed)
    r = measure(ctx, arr["instances"], moves(rs, arr["instances"], idx, reach))
    r["nodes"] = ctx.build_info()["nodes"]
    ctx.close()
    return r


def trace_ms(ctx, sc, w=1920, h=1080):
    ctx.resize(w, h)
    ctx.reset_stats()
    ctx.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=0, spp_total=1, max_depth=4))
    ctx.synchronize()
    return ctx.stats()["ms_trace_closest"]


def main():
    out = {}
    sc = scenes.kitchen_standin()
    arr = dict(sc.arrays())
    mesh = np.nonzero(arr["instances"]["type"] == S.INSTANCE_MESH)[0]
    out["kitchen_baked_one_moved"] = case(arr, mesh[7:8], HALF_ROOM, 1)
    out["kitchen_baked_all_moved"] = case(arr, mesh, HALF_ROOM, 2)
    out["kitchen_bake0_one_moved"] = case(arr, mesh[7:8], HALF_ROOM, 3, [("bake_world", 0)])
    out["kitchen_bake0_all_moved"] = case(arr, mesh, HALF_ROOM, 4, [("bake_world", 0)])
    print(json.dumps({"progress": "kitchen"}), file=sys.stderr, flush=True)
    # the trace through an updated hierarchy: after one instance moved, after every instance moved by up to half the room, and through a rebuilt one
    # (timing on: per-launch hipEvent spans)
    one = moves(np.random.RandomState(5), arr["instances"], mesh[7:8], HALF_ROOM)
    big = moves(np.random.RandomState(5), arr["instances"], mesh, HALF_ROOM)
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)
    ctx.set_scene(arr)
    tr = {"built": float(np.median([trace_ms(ctx, sc) for _ in range(3)]))}
    for name, table in (("one_moved_updated", one), ("all_moved_updated", big)):
        ctx.update_accel(table)
        assert ctx.build_info()["refit"] == 2
        tr[name] = float(np.median([trace_ms(ctx, sc) for _ in range(3)]))
    ctx.build_accel()
    tr["all_moved_rebuilt"] = float(np.median([trace_ms(ctx, sc) for _ in range(3)]))
    ctx.close()
    out["kitchen_ms_trace_closest_1080p"] = tr
    # 10^5 instances (tests/test_gpu_fullsize.py)
    rs = np.random.RandomState(9)
    s2 = S.Scene()
    mat = s2.addMaterial(S.MAT_DIFFUSE, (0.7, 0.7, 0.7))
    pos, tris = scenes._grid_mesh(scenes._sphere_fn(rs, 0.1), 5, 4)
    m = scenes._add_mesh(s2, pos, tris)
    N = 100_000
    P = rs.uniform(-40, 40, (N, 3))
    for k in range(N):
        sx = rs.uniform(0.1, 0.4)
        s2.createInstance(S.INSTANCE_MESH, m, mat, S.translate(P[k]) @ S.scale((sx, sx * rs.uniform(0.5, 2.0), sx)))
    a2 = dict(s2.arrays())
    allk = np.arange(N)
    out["inst1e5_baked_all_moved"] = case(a2, allk, np.array([5.0, 5.0, 5.0]), 6)
    out["inst1e5_bake0_all_moved"] = case(a2, allk, np.array([5.0, 5.0, 5.0]), 7, [("bake_world", 0)])
    print(json.dumps({"progress": "1e5"}), file=sys.stderr, flush=True)
    # a groom cut into 8 prims under transforms of their own: curve BLASes under a TLAS
    a3 = dict(scenes.hair_standin(n_prims=8, prim_offset=0.05).arrays())
    curve = np.nonzero(a3["instances"]["type"] == S.INSTANCE_CURVE)[0]
    out["hair8_all_prims_moved"] = case(a3, curve, np.array([0.2, 0.2, 0.2]), 8)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
