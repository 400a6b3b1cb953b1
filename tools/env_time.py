"""The environment light's costs (DESIGN.md section 2 "Environment light", docs/LOG.md).  usage (GPU box): python tools/env_time.py

1. Table build, 2048 x 1024 and 8192 x 4096: skh_get_environment_info's ms (median of 3) and the bytes the three kernels move per ms (12 B read + 16 B
   written per texel by k_env_rows, + 4 B of conditional CDF, + 16 B read and 4 B written by k_env_normalise = 52 B per texel) next to the copy rate
   skh_probe_memory reports on the same box.
2. Kitchen stand-in, 1080p, 4 bounces, 64 sub-frames in one pass, the legs alternated, each in a child process of its own: without an environment,
   with a 2048 x 1024 sky, without, with -- the repeats give the spread of a leg against itself.  Per leg and repeat: the kernels' ms per frame, ms_shade,
   ms_trace_closest / _shadow, rays, Mray/s, ms_shade per launch.  (The run without an environment launches k_shade<false, false>, the kernel of before the
   environment existed: compare it with `bench.py` of the parent commit on the same box.)  Prints one JSON object."""
import json
import os
import subprocess
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H, SPP, DEPTH = 1920, 1080, 64, 4


def sky(w, h, seed=5):
    """a smooth gradient plus a small sun 10^4 times brighter (what tests/envref.py builds, restated: tools do not import tests)"""
    rs = np.random.RandomState(seed)
    up = np.cos((np.arange(h) + 0.5) / h * np.pi)[:, None]
    base = np.where(up > 0, 0.3 + 0.7 * (1 - up) ** 3, 0.05 + 0.1 * (1 + up))
    rgb = np.repeat((base[..., None] * rs.uniform(0.4, 1.0, 3)[None, None, :]), w, axis=1)
    iy, ix, n = int(h * 0.25), int(w * 0.6), max(1, min(3, h // 32))
    rgb[iy:iy + n, ix:ix + n] *= 1e4
    return np.ascontiguousarray(rgb, np.float32)


def leg(with_env):
    from strelka_amd import capi, scene as S, scenes

    sc = scenes.kitchen_standin()
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)
    ctx.set_scene(sc.arrays())
    if with_env:
        ctx.set_environment(sky(2048, 1024), (0.5, 0.5, 0.5))
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
    from strelka_amd import capi

    ctx = capi.Context(0)
    gbps, _ = ctx.probe_memory(0, 1 << 30)
    out = {"stream_copy_GBps": round(gbps, 1)}
    for w, h in ((2048, 1024), (8192, 4096)):
        m = sky(w, h)
        ms = []
        for _ in range(3):
            ctx.set_environment(m)
            ms.append(ctx.environment_info()["ms_build"])
        moved = w * h * 52
        out[f"{w}x{h}"] = {"ms_build": round(float(np.median(ms)), 3), "ms_all": [round(x, 3) for x in ms], "table_bytes": ctx.environment_info()["bytes"],
                           "GB_moved_per_s": round(moved / np.median(ms) / 1e6, 1)}
        ctx.set_environment(None)
    ctx.close()
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--leg":
        print(json.dumps(leg(sys.argv[2] == "env")))
        return

    def child(which):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which], capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise SystemExit(f"leg {which} failed with {r.returncode}: {r.stderr[-1500:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"build": build_times(), "kitchen_1080p_64spp": {}}
    print(json.dumps({"progress": "build"}), file=sys.stderr, flush=True)
    for name, which in (("noenv_a", "noenv"), ("env_a", "env"), ("noenv_b", "noenv"), ("env_b", "env")):
        out["kitchen_1080p_64spp"][name] = child(which)
        print(json.dumps({"progress": name}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
