"""The costs of emissive meshes (DESIGN.md section 2 "Emissive meshes", docs/LOG.md).  usage (GPU box): python tools/emit_time.py

1. Table build: skh_get_emitter_info's ms (median of 3 builds, each after skh_set_emission marked the table stale), entries and bytes, for a quad of
   73 728 emissive triangles and for the kitchen stand-in with materials 1 ... 8 emissive (a few hundred instances, some millions of triangles).
2. Kitchen stand-in, 1080p, 4 bounces, 64 sub-frames in one pass, the legs alternated, each in a child process of its own: without emission, with it,
   without, with.  Per leg and repeat: the kernels' ms per frame, ms_shade, ms_trace_closest / _shadow, rays, Mray/s, ms_shade per launch.  (The run
   without emission launches k_shade<false, false, false>, the kernel of before: compare it with `bench.py` of the parent commit on the same box.)
Prints one JSON object."""
import json
import os
import subprocess
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H, SPP, DEPTH = 1920, 1080, 64, 4
EMISSIVE = range(1, 9)  # materials of the kitchen stand-in that emit in the `emit` legs
LE = (0.5, 0.45, 0.35)


def kitchen_emission(arr):
    em = np.zeros((len(arr["materials"]), 3), np.float32)
    em[list(EMISSIVE)] = LE
    return em


def quad_scene(nx=256, nz=144):
    """a 1.0 x 0.5625 quad of 2 nx nz triangles facing down, interior vertices jittered (what tests/test_gpu_emit.py builds, restated: tools do not import tests)"""
    from strelka_amd import scene as S

    rs = np.random.RandomState(5)
    gx, gz = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="ij")
    inner = (gx > 0) & (gx < nx) & (gz > 0) & (gz < nz)
    x = gx * 16.0 + np.where(inner, rs.randint(-2, 3, gx.shape), 0)
    z = gz * 16.0 + np.where(inner, rs.randint(-2, 3, gz.shape), 0)
    P = np.stack([x / 4096.0 - 0.5, np.full(x.shape, 1.5), z / 4096.0 - 0.28125], -1)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    tris = np.stack([np.stack([a, b, c], 2), np.stack([a, c, d], 2)], 2).reshape(-1, 3, 3).astype(np.float32)
    sc = S.Scene()
    m = sc.addMaterial(S.MAT_DIFFUSE, (0.0, 0.0, 0.0), emission=(3.0, 2.0, 1.0))
    vb, ib = S.deindex(tris.reshape(-1, 3), np.arange(3 * len(tris)).reshape(-1, 3))
    sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, ib), m, np.eye(4))
    return sc


def leg(with_emit):
    from strelka_amd import capi, scene as S, scenes

    sc = scenes.kitchen_standin()
    arr = sc.arrays()
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)
    ctx.set_scene(arr)
    if with_emit:
        ctx.set_emission(kitchen_emission(arr))
    ctx.resize(W, H)
    p = S.frame_params(sc.getCamera(), W, H, subframe_index=0, spp_total=SPP, max_depth=DEPTH)
    out = []
    for rep in range(3):  # the first is the warm-up
        ctx.reset_stats()
        ctx.render_subframes(p, SPP)
        ctx.synchronize()
        st = ctx.stats()
        ms = st["ms_trace_closest"] + st["ms_trace_shadow"] + st["ms_shade"] + st["ms_raygen"] + st["ms_accumulate"]
        rays = st["rays_radiance"] + st["rays_shadow"]
        out.append({"ms_kernels": round(ms, 3), "ms_shade": round(st["ms_shade"], 3), "ms_trace_closest": round(st["ms_trace_closest"], 3),
                    "ms_trace_shadow": round(st["ms_trace_shadow"], 3), "rays_shadow_per_frame": st["rays_shadow"], "rays_radiance_per_frame": st["rays_radiance"],
                    "mrays_per_s": round(rays / ms / 1e3, 1), "ms_shade_per_launch": round(st["ms_shade"] / max(1, st["launches_shade"]), 4)})
    ctx.close()
    return out[1:]


def build_times():
    from strelka_amd import capi, scenes

    ctx = capi.Context(0)
    out = {}
    kitchen = scenes.kitchen_standin().arrays()
    for name, arr, em in (("quad_73728", quad_scene().arrays(), None), ("kitchen_materials_1_to_8", kitchen, kitchen_emission(kitchen))):
        ctx.set_scene(arr, build=False)  # (the table needs no acceleration structure)
        em = arr["emission"] if em is None else em
        ms = []
        for _ in range(3):
            ctx.set_emission(em)
            ms.append(ctx.emitter_info()["ms_build"])
        info = ctx.emitter_info()
        out[name] = {"ms_build": round(float(np.median(ms)), 3), "ms_all": [round(x, 3) for x in ms], "triangles": info["triangles"], "instances": info["instances"],
                     "table_bytes": info["bytes"], "sum_w": info["sum_w"]}
    ctx.close()
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--leg":
        print(json.dumps(leg(sys.argv[2] == "emit")))
        return

    def child(which):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which], capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise SystemExit(f"leg {which} failed with {r.returncode}: {r.stderr[-1500:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"build": build_times(), "kitchen_1080p_64spp": {}}
    print(json.dumps({"progress": "build"}), file=sys.stderr, flush=True)
    for name, which in (("plain_a", "plain"), ("emit_a", "emit"), ("plain_b", "plain"), ("emit_b", "emit")):
        out["kitchen_1080p_64spp"][name] = child(which)
        print(json.dumps({"progress": name}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
