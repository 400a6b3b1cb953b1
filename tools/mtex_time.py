"""The cost of material textures in k_shade (DESIGN.md section 2 "Material textures", docs/LOG.md).  usage (GPU box): python tools/mtex_time.py

Kitchen stand-in, 1080p, 4 bounces, 64 sub-frames in one pass, three legs, alternated, each in a child process of its own, twice:
  plain     no map: no texture, no table -- k_shade<false, false, false, false>, the kernel of before (compare it with `bench.py` of the parent commit on the same box)
  orm       ONE shared 1024 x 1024 map on every PBR material, roughness = g, metallic = b: one look-up per PBR triangle hit
  separate  a roughness map and a metallic map, 1024 x 1024 each, on every PBR material: two look-ups
The stand-in's vertices carry no uvs (all of them would read one texel): the mapped legs give every vertex uv = 0.5 (x, z) of its object-space position, so that
neighbouring hits read neighbouring texels and distant ones distant texels, as a parametrised asset does.  The maps are noise around 0.5 with scale 0.5 and the
material's constant as the centre (bias = constant - 0.25): the BSDF lobes keep their width on average and the ray counts stay comparable.
Per leg and repeat: the kernels' ms per frame, ms_shade, ms_trace_closest / _shadow, rays, Mray/s, ms_shade per launch.  Prints one JSON object."""
import json
import os
import subprocess
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H, SPP, DEPTH = 1920, 1080, 64, 4
SIZE = 1024


def noise_map(seed):
    return np.random.RandomState(seed).randint(0, 256, (SIZE, SIZE, 4)).astype(np.uint8)


def leg(which):
    from strelka_amd import capi, scene as S, scenes

    sc = scenes.kitchen_standin()
    arr = sc.arrays()
    n_pbr = int((arr["materials"]["type"] == S.MAT_PBR).sum())
    if which != "plain":
        v = arr["vertices"]
        v["uv"] = S.pack_uv(np.clip(v["pos"][:, [0, 2]] * np.float32(0.5), -10.0, 10.0))
        arr["textures"] = [noise_map(1)] if which == "orm" else [noise_map(1), noise_map(2)]
        t = np.zeros(len(arr["materials"]), S.MATERIAL_TEXTURES)
        t["emission_channel"] = S.EMISSION_RGB
        t["roughness_scale"] = t["metallic_scale"] = 0.5
        pbr = arr["materials"]["type"] == S.MAT_PBR
        t["roughness_bias"] = arr["materials"]["roughness"] - np.float32(0.25)
        t["metallic_bias"] = arr["materials"]["metallic"] - np.float32(0.25)
        t["roughness_texture"][pbr] = 1
        t["metallic_texture"][pbr] = 1 if which == "orm" else 2
        t["roughness_channel"], t["metallic_channel"] = (1, 2) if which == "orm" else (0, 0)
        arr["material_textures"] = t
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)
    ctx.set_scene(arr)
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
                    "mrays_per_s": round(rays / ms / 1e3, 1), "ms_shade_per_launch": round(st["ms_shade"] / max(1, st["launches_shade"]), 4), "pbr_materials": n_pbr})
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

    out = {"kitchen_1080p_64spp": {}}
    for rnd in ("a", "b"):
        for which in ("plain", "orm", "separate"):
            out["kitchen_1080p_64spp"][f"{which}_{rnd}"] = child(which)
            print(json.dumps({"progress": f"{which}_{rnd}"}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
