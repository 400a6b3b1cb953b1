"""The cost of fractional opacity (DESIGN.md section 2 "Fractional opacity", docs/LOG.md).  usage (GPU box): python tools/blend_time.py [--once]

The scene of tools/cutout_time.py: the kitchen stand-in, 1080p, 4 bounces, 16 sub-frames in one pass, plus its CARD LAYER (400 cards of 32 triangles).
Four legs, each in a child process of its own, twice, alternated:
  plain     the stand-in without the cards -- the layer deleted: the kernels of before (compare it with `bench.py` of the parent commit on the same box)
  blend     the cards with a blend table, a = 0.5 on every card: k_cutout's BLEND build and its continuation rounds, radiance rays gambled, shadow rays scaled
  masked    the same layer as a threshold cutout (cutout_time.py's `masked`): the stage's build without BLEND
  opaque    the same cards without a table: what the layer costs as plain geometry
Per leg and repeat: the wall time of the frame, the kernels' ms by class (the stage's launches are inside the trace classes of their side), rays, and the
stage's counters.  Prints one JSON object."""
import json
import math
import os
import subprocess
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from cutout_time import CARDS, DEPTH, H, SPP, W, block_alpha, card_mesh  # noqa: E402


def leg(which):
    from strelka_amd import capi, scene as S, scenes

    sc = scenes.kitchen_standin()
    alpha = block_alpha()
    if which != "plain":
        tex = np.random.RandomState(9).randint(0, 256, (8, 8, 4)).astype(np.uint8)
        tex[..., 3] = np.kron(alpha, np.ones((2, 2), np.uint8))
        tid = sc.addTexture(tex)
        how = {"masked": {"opacity_texture": tid, "opacity_channel": 3, "opacity_threshold": 0.5},
               "blend": {"opacity_scale": 0.0, "opacity_bias": 0.5, "opacity_blend": True}}.get(which, {})
        mat = sc.addMaterial(S.MAT_DIFFUSE, (0.3, 0.6, 0.25), base_color_texture=tid, **how)
        mesh = card_mesh(sc, S, alpha, False)
        rs = np.random.RandomState(77)
        for _ in range(CARDS):
            pos = (rs.uniform(-4.2, 4.2), rs.uniform(0.6, 3.2), rs.uniform(-2.3, 2.3))
            xf = S.translate(pos) @ S.rotate((0, 1, 0), rs.uniform(0, 2 * math.pi)) @ S.rotate((1, 0, 0), math.radians(90)) @ S.scale((0.5, 1.0, 0.5))
            sc.createInstance(S.INSTANCE_MESH, mesh, mat, xf)
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)
    ctx.set_scene(sc.arrays())
    ctx.resize(W, H)
    p = S.frame_params(sc.getCamera(), W, H, subframe_index=0, spp_total=SPP, max_depth=DEPTH)
    out = []
    for rep in range(3):  # the first is the warm-up
        ctx.reset_stats()
        t0 = time.perf_counter()
        ctx.render_subframes(p, SPP)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st, ci, bi = ctx.stats(), ctx.cutout_info(), ctx.blend_info()
        ms = st["ms_trace_closest"] + st["ms_trace_shadow"] + st["ms_shade"] + st["ms_raygen"] + st["ms_accumulate"]
        out.append({"ms_frame_wall": round(wall / SPP, 3), "ms_kernels_per_frame": round(ms / SPP, 3), "ms_trace_closest": round(st["ms_trace_closest"] / SPP, 3),
                    "ms_trace_shadow": round(st["ms_trace_shadow"] / SPP, 3), "ms_shade": round(st["ms_shade"] / SPP, 3), "rays_radiance": st["rays_radiance"],
                    "rays_shadow": st["rays_shadow"], "mray_per_s": round((st["rays_radiance"] + st["rays_shadow"]) / (ms * 1e3), 1) if ms > 0 else 0.0,
                    "continued_closest": ci["continued_closest"], "continued_shadow": ci["continued_shadow"], "passed_radiance": bi["passed_radiance"],
                    "crossed_shadow": bi["crossed_shadow"], "accepted_by_cap": ci["accepted_by_cap"] + bi["accepted_by_cap"], "stage_bytes": bi["bytes"],
                    "blend_instances": bi["instances"], "cutout_instances": ci["instances"]})
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
        for which in ("plain", "blend", "masked", "opaque"):
            out[key][f"{which}_{rnd}"] = child(which)
            print(json.dumps({"progress": f"{which}_{rnd}"}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
