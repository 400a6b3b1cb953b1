"""The cost and the gain of adaptive sampling (DESIGN.md section 2 "Adaptive sampling", docs/LOG.md).  usage (GPU box): python tools/adaptive_time.py [--once] [--only thr]

The bench workload at its own size: the kitchen stand-in, 1920 x 1080, 4 bounces, 64 sub-frames in one skh_render_subframes call.  Legs, each in a child
process of its own, twice, alternated:
  off        the feature never turned on: the kernels of before (compare it with `bench.py` of the parent commit on the same box)
  overhead   on, min_samples = spp_total: nothing can freeze -- the frame of `off` plus k_adapt_moments and one check: the pure overhead
  thr_X      on at relative standard error X (dark level: radiance 0.05 under the frame's exposure; min_samples 16, interval 8): time, rays, tiles' observation
             counts, and the RMS difference in tonemapped luminance to the full frame of the SAME run (the accumulator after all 64 sub-frames)
  calls_off / calls_on   one skh_render_subframe call per sub-frame, the reference caller's pattern: with the feature on the library traces nothing ahead
             (min_samples = spp_total: the same rays) -- the per-call cost of that
Per leg and repeat: wall time of the frame, rays.  Prints one JSON object."""
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H, SPP, DEPTH = 1920, 1080, 64, 4
THRESHOLDS = (0.1, 0.3, 1.0)
DARK_RADIANCE, MIN_SAMPLES, INTERVAL = 0.05, 16, 8


def luma(img, exposure):
    c = img[..., :3] * exposure
    t = c / (c + np.float32(1.0))
    return np.float32(0.2126) * t[..., 0] + np.float32(0.7152) * t[..., 1] + np.float32(0.0722) * t[..., 2]


def leg(which):
    from strelka_amd import capi, scene as S, scenes

    sc = scenes.kitchen_standin()
    ctx = capi.Context(0)
    ctx.set_scene(sc.arrays())
    ctx.resize(W, H)
    p = S.frame_params(sc.getCamera(), W, H, subframe_index=0, spp_total=SPP, max_depth=DEPTH)
    exposure = np.asarray(p["exposure"], np.float32)
    dark = capi.adaptive_dark_level(DARK_RADIANCE, exposure)

    def frame(calls=False):
        ctx.reset_stats()
        t0 = time.perf_counter()
        if calls:
            for i in range(SPP):
                ctx.render_subframe(S.frame_params(sc.getCamera(), W, H, subframe_index=i, spp_total=SPP, max_depth=DEPTH))
        else:
            ctx.render_subframes(p, SPP)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx.stats()
        return {"ms_frame": round(wall, 3), "rays": st["rays_radiance"] + st["rays_shadow"]}

    full = None
    if which.startswith("thr_"):
        frame()
        full = luma(ctx.read_accum(), exposure)  # the full frame of this run
        ctx.set_adaptive(float(which[4:]), dark, MIN_SAMPLES, INTERVAL)
    elif which in ("overhead", "calls_on"):
        ctx.set_adaptive(0.05, dark, SPP, INTERVAL)
    out = []
    for rep in range(3):  # the first is the warm-up
        r = frame(which.startswith("calls"))
        if full is not None:
            info = ctx.adaptive_info()
            d = luma(ctx.read_accum(), exposure).astype(np.float64) - full
            n = ctx.read_adaptive()[..., 0]
            r.update({"rms_ldr_luminance": float(np.sqrt((d * d).mean())), "mean_ldr_luminance": float(full.mean()), "active_tiles": info["active_tiles"],
                      "tiles": info["tiles"], "checks": info["checks"], "mean_observations": round(float(n.mean()), 2), "min_observations": info["min_observations"],
                      "pixel_observations_saved": info["pixel_observations_saved"]})
        out.append(r)
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

    key = "kitchen_1080p_%dspp" % SPP
    out = {key: {}}
    for rnd in ("a",) if "--once" in sys.argv else ("a", "b"):
        for which in ("off", "overhead") + tuple("thr_%g" % t for t in THRESHOLDS) + ("calls_off", "calls_on"):
            if "--only" in sys.argv and not which.startswith(sys.argv[sys.argv.index("--only") + 1]):
                continue
            out[key][f"{which}_{rnd}"] = child(which)
            print(json.dumps({"progress": f"{which}_{rnd}"}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
