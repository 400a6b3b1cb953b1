"""The costs of light shapes (DESIGN.md section 2 "Light shapes", docs/LOG.md).  usage (GPU box): python tools/lightshape_time.py [--out profiles/lightshape_time.json]

scenes.spot_room() at 1080p, 4 bounces, 32 sub-frames in one pass, the legs alternated, each in a child process of its own: the scene with its shapes (a
sampled disk, a coned sphere light, a coned rect light: the LSHAPE builds of k_shade) and the same scene with the table removed (the kernels of before; the disk
is then the reference's: never sampled, lit only where a BSDF ray meets it).  Per leg and repeat: the kernels' ms per frame, ms_shade and ms_shade per launch,
the trace kernels' ms, rays, shadow rays per camera sample, Mray/s.  Prints one JSON object (and writes it to --out)."""
import json
import os
import subprocess
import sys

sys.path.insert(0, ".")

W, H, SPP, DEPTH = 1920, 1080, 32, 4


def leg(shaped):
    from strelka_amd import capi, scene as S, scenes

    sc = scenes.spot_room()
    arr = sc.arrays()
    if not shaped:
        arr = {k: v for k, v in arr.items() if k != "light_shapes"}
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)
    ctx.set_scene(arr)
    info = ctx.light_shape_info()
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
                    "ms_trace_shadow": round(st["ms_trace_shadow"], 3), "rays_shadow": st["rays_shadow"], "rays_radiance": st["rays_radiance"],
                    "shadow_rays_per_sample": round(st["rays_shadow"] / float(W * H * SPP), 4), "mrays_per_s": round(rays / ms / 1e3, 1),
                    "ms_shade_per_launch": round(st["ms_shade"] / max(1, st["launches_shade"]), 4), "shapes_in_use": info})
    ctx.close()
    return out[1:]


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--leg":
        print(json.dumps(leg(sys.argv[2] == "shaped")))
        return

    def child(which):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit(f"leg {which} failed with {r.returncode}: {r.stderr[-1500:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"scene": "spot_room", "width": W, "height": H, "spp": SPP, "max_depth": DEPTH, "legs": {}}
    for name, which in (("plain_a", "plain"), ("shaped_a", "shaped"), ("plain_b", "plain"), ("shaped_b", "shaped")):
        out["legs"][name] = child(which)
        print(json.dumps({"progress": name}), file=sys.stderr, flush=True)
    text = json.dumps(out)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
