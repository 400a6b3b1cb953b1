"""The cost of cutouts (DESIGN.md section 2 "Cutouts", docs/LOG.md).  usage (GPU box): python tools/cutout_time.py [--once]

Kitchen stand-in, 1080p, 4 bounces, 16 sub-frames in one pass, plus a CARD LAYER: 400 cards of 32 triangles (4 x 4 cells, unshared vertices, every triangle's
three vertices at the centre of one 2 x 2-texel block of an 8 x 8 texture whose alpha is 0 or 255 per block -- about half of the triangles are cut), 0.5 x 0.5
units each, upright at random places and headings in the room's free volume between the floor objects and the ceiling lights.  Four legs, each in a child
process of its own, twice, alternated:
  plain     the stand-in without the cards: the kernels of before (compare it with `bench.py` of the parent commit on the same box)
  masked    the cards with the cutout table: k_cutout and its continuation rounds between trace and shade, closest-hit launches in the any-hit launch's place
  opaque    the same cards without the table: what the layer costs as plain geometry
  removed   the cut triangles taken out of the geometry: the picture of `masked`, by the kernels of before
Per leg and repeat: the wall time of the frame, the kernels' ms by class (the cutout stage's launches are inside the trace classes of their side), rays, and the
rays continued.  Prints one JSON object."""
import json
import math
import os
import subprocess
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H, SPP, DEPTH = 1920, 1080, 16, 4
CARDS = 400


def block_alpha():
    a = np.random.RandomState(5).randint(0, 2, (4, 4)).astype(np.uint8) * 255
    a[0, 0], a[3, 3] = 0, 255
    return a


def card_mesh(sc, S, alpha, keep_only):
    tris, uvs = [], []
    cell = 0.25
    t = 0
    for cz in range(4):
        for cx in range(4):
            x0, z0 = -0.5 + cx * cell, -0.5 + cz * cell
            a, b, c, d = (x0, 0.0, z0 + cell), (x0 + cell, 0.0, z0 + cell), (x0 + cell, 0.0, z0), (x0, 0.0, z0)
            for tri in ((a, b, c), (a, c, d)):
                k = (5 * t + 3) % 16
                t += 1
                if keep_only and alpha[k // 4, k % 4] == 0:
                    continue
                tris.append(tri)
                uvs.append(((2 * (k % 4) + 1) / 8.0, (2 * (k // 4) + 1) / 8.0))
    tris = np.float32(tris)
    vb, ib = S.deindex(tris.reshape(-1, 3), np.arange(3 * len(tris)).reshape(-1, 3))
    vb["uv"] = S.pack_uv(np.repeat(np.float32(uvs), 3, axis=0))
    return sc.createMesh(vb, ib)


def leg(which):
    from strelka_amd import capi, scene as S, scenes

    sc = scenes.kitchen_standin()
    alpha = block_alpha()
    n_mat = len(sc.mMaterials)
    if which != "plain":
        tex = np.random.RandomState(9).randint(0, 256, (8, 8, 4)).astype(np.uint8)
        tex[..., 3] = np.kron(alpha, np.ones((2, 2), np.uint8))
        tid = sc.addTexture(tex)
        mat = sc.addMaterial(S.MAT_DIFFUSE, (0.3, 0.6, 0.25), base_color_texture=tid,
                             **({"opacity_texture": tid, "opacity_channel": 3, "opacity_threshold": 0.5} if which == "masked" else {}))
        mesh = card_mesh(sc, S, alpha, which == "removed")
        rs = np.random.RandomState(77)
        for _ in range(CARDS):
            pos = (rs.uniform(-4.2, 4.2), rs.uniform(0.6, 3.2), rs.uniform(-2.3, 2.3))
            xf = S.translate(pos) @ S.rotate((0, 1, 0), rs.uniform(0, 2 * math.pi)) @ S.rotate((1, 0, 0), math.radians(90)) @ S.scale((0.5, 1.0, 0.5))
            sc.createInstance(S.INSTANCE_MESH, mesh, mat, xf)
        n_mat += 1
    arr = sc.arrays()
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)
    ctx.set_scene(arr)
    ctx.resize(W, H)
    p = S.frame_params(sc.getCamera(), W, H, subframe_index=0, spp_total=SPP, max_depth=DEPTH)
    out = []
    for rep in range(3):  # the first is the warm-up
        ctx.reset_stats()
        t0 = time.perf_counter()
        ctx.render_subframes(p, SPP)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st, info = ctx.stats(), ctx.cutout_info()
        ms = st["ms_trace_closest"] + st["ms_trace_shadow"] + st["ms_shade"] + st["ms_raygen"] + st["ms_accumulate"]
        out.append({"ms_frame_wall": round(wall / SPP, 3), "ms_kernels_per_frame": round(ms / SPP, 3), "ms_trace_closest": round(st["ms_trace_closest"] / SPP, 3),
                    "ms_trace_shadow": round(st["ms_trace_shadow"] / SPP, 3), "ms_shade": round(st["ms_shade"] / SPP, 3), "rays_radiance": st["rays_radiance"],
                    "rays_shadow": st["rays_shadow"], "continued_closest": info["continued_closest"], "continued_shadow": info["continued_shadow"],
                    "accepted_by_cap": info["accepted_by_cap"], "cutout_bytes": info["bytes"], "cutout_instances": info["instances"]})
    ctx.close()
    return out[1:]


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--leg":
        print(json.dumps(leg(sys.argv[2])))
        return

    def child(which):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which], capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise SystemExit(f"leg {which} failed with {r.returncode}: {r.stderr[-1500:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    key = "kitchen_cards_1080p_%dspp" % SPP
    out = {key: {}}
    for rnd in ("a",) if "--once" in sys.argv else ("a", "b"):
        for which in ("plain", "masked", "opaque", "removed"):
            out[key][f"{which}_{rnd}"] = child(which)
            print(json.dumps({"progress": f"{which}_{rnd}"}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
