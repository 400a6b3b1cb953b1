"""Renders one of the stand-in scenes, or a glTF file, on the GPU and writes a tonemapped PNG (usage: render_png.py kitchen|cornell|hair|FILE.gltf|FILE.glb W H spp depth [exposure_scale] [out.png] [--env FILE.hdr [--env-rotate DEG]] [--alpha-blend] [--adaptive THR [--adaptive-min N --adaptive-interval K]] [--sample-map FILE.png]:
--env lights the scene with a lat-long Radiance map as its dome light, --env-rotate turns the dome about +Y).  A scene whose materials emit
(Scene.addMaterial(emission=...), a glTF emissiveFactor) needs no flag: its arrays carry "emission" and Context.set_scene forwards it.  A glTF file is
loaded with material_textures=True: its metallicRoughnessTexture and emissiveTexture are rendered (arrays()["material_textures"]).
--alpha-blend: a glTF file's alphaMode BLEND materials are rendered with fractional opacity (load_gltf(alpha_blend=True)) instead of as glass.
--adaptive THR: adaptive sampling -- a tile stops at relative standard error THR of its pixels' tonemapped luminance (checked after --adaptive-min launches,
default 16, and every --adaptive-interval after, default 8; dark level: radiance 0.05 under the frame's exposure); --sample-map FILE.png writes the per-pixel
observation count as a grey image (white = spp).
--aov NAME=FILE.png (repeatable): a first-hit plane of the same camera through the pixel centres (skh_render_aovs), NAME one of ids, depth, normal, geom_normal,
position, albedo, uv: normals as (N + 1) / 2 (black where nothing is hit), depth normalised over the hits (near white, far black), ids as hashed colours of
(instance, primitive), albedo, position and uv written straight (clipped to 0 ... 1 by the PNG).
--denoise [LEVELS] (after the positional arguments, out.png among them): the picture once more through skh_denoise -- LEVELS levels, default 5, scene.denoise_params' defaults for this
image and scene --, written next to the raw one as <out>_denoised.png."""
import sys, numpy as np
sys.path.insert(0, ".")
import math
import torch
from strelka_amd import capi, gltf, hdr, scene as S, scenes, png
env_file = env_deg = None
alpha_blend = "--alpha-blend" in sys.argv
if alpha_blend:
    sys.argv.remove("--alpha-blend")
aov_out = []
while "--aov" in sys.argv:
    k = sys.argv.index("--aov")
    aov_out.append(tuple(sys.argv[k + 1].split("=", 1)))
    del sys.argv[k:k + 2]
denoise_levels = None
if "--denoise" in sys.argv:
    k = sys.argv.index("--denoise")
    has_value = k + 1 < len(sys.argv) and sys.argv[k + 1].isdigit() and k >= 6  # (after the five positional arguments: a number there is LEVELS)
    denoise_levels = int(sys.argv[k + 1]) if has_value else 5
    del sys.argv[k:k + (2 if has_value else 1)]
opts = {}
for flag in ("--env-rotate", "--env", "--adaptive-min", "--adaptive-interval", "--adaptive", "--sample-map"):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        val = sys.argv[k + 1]
        del sys.argv[k:k + 2]
        if flag == "--env":
            env_file = val
        elif flag == "--env-rotate":
            env_deg = float(val)
        else:
            opts[flag] = val
if denoise_levels is not None and len(sys.argv) <= 7:
    sys.exit("--denoise writes next to the raw picture: give exposure_scale and out.png")
name = sys.argv[1]; W, H, spp, depth = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
if name.lower().endswith((".gltf", ".glb")):
    sc, name = gltf.load_gltf(name, material_textures=True, alpha_blend=alpha_blend), name.replace("/", "_")
else:
    sc = {"kitchen": scenes.kitchen_standin, "cornell": scenes.cornell_box, "hair": scenes.hair_standin}[name]()
if env_file:
    a = math.radians(env_deg or 0.0)  # world -> environment: a turn of the dome by +a about Y is a turn of the directions by -a
    sc.setEnvironment(hdr.load_hdr(env_file), world_to_env=[[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
ctx = capi.Context(0); ctx.set_scene(sc.arrays()); ctx.resize(W, H)
p = S.frame_params(sc.getCamera(), W, H, subframe_index=0, spp_total=spp, max_depth=depth)
if "--adaptive" in opts:
    ctx.set_adaptive(float(opts["--adaptive"]), capi.adaptive_dark_level(0.05, p["exposure"]), int(opts.get("--adaptive-min", 16)), int(opts.get("--adaptive-interval", 8)))
ctx.render_subframes(p, spp, None)
if "--adaptive" in opts:
    print("adaptive:", ctx.adaptive_info(), "rays", ctx.stats()["rays_radiance"] + ctx.stats()["rays_shadow"])
if "--sample-map" in opts:
    n = ctx.read_adaptive()[..., 0] if "--adaptive" in opts else np.full((H, W), spp, np.float32)
    png.save_png(opts["--sample-map"], np.repeat((n / np.float32(spp))[..., None], 3, -1), flipped=True)
if aov_out:
    plane_of = {"ids": "ids", "depth": "hit", "normal": "normal", "geom_normal": "geom_normal", "position": "position", "albedo": "albedo", "uv": "texcoord"}
    a = ctx.render_aovs(S.aov_params(sc.getCamera(), W, H), tuple({"ids"} | {plane_of[n] for n, _ in aov_out}))
    hit = a["ids"][..., 3] != 0
    surface = ((a["ids"][..., 3] == 1) | (a["ids"][..., 3] == 2))[..., None]
    for n, path in aov_out:
        if n == "ids":
            h = (a["ids"][..., 0] * np.uint32(0x9E3779B1)) ^ (a["ids"][..., 1] * np.uint32(0x85EBCA6B))
            h ^= h >> np.uint32(15)
            rgb = np.stack([(h >> np.uint32(s)) & np.uint32(255) for s in (0, 8, 16)], -1).astype(np.float32) / 255.0 * hit[..., None]
        elif n == "depth":
            d = a["hit"][..., 3]
            lo, hi = (float(d[hit].min()), float(d[hit].max())) if hit.any() else (0.0, 1.0)
            rgb = np.repeat(np.where(hit, 1.0 - (d - lo) / max(hi - lo, 1e-30), 0.0)[..., None], 3, -1).astype(np.float32)
        elif n in ("normal", "geom_normal"):
            rgb = np.where(surface, (a[n][..., :3] + np.float32(1.0)) * np.float32(0.5), np.float32(0.0))
        else:
            rgb = a[plane_of[n]][..., :3]
        png.save_png(path, np.ascontiguousarray(rgb, np.float32), flipped=True)
        print("wrote", n, path)
img = torch.from_numpy(ctx.read_accum()).cuda()
e = S.default_exposure() * np.float32(float(sys.argv[6]) if len(sys.argv) > 6 else 1.0)
ctx.tonemap(img.data_ptr(), W, H, 1, e, 2.2)   # Reinhard + gamma, as the reference's post chain
png.save_png((sys.argv[7] if len(sys.argv) > 7 else f"gpurun_out/{name}.png"), img.cpu().numpy()[..., :3], flipped=True)
print("wrote", name, float(img.mean()))
if denoise_levels is not None:
    # the same linear image through skh_denoise (guides through the pixel centres, default parameters), then the same post chain, next to the raw picture
    raw, arr = ctx.read_accum(), sc.arrays()
    guides = ctx.render_guides(S.aov_params(sc.getCamera(), W, H))
    dp = S.denoise_params(W, H, levels=denoise_levels, scene=arr, image=raw, guides=guides)
    den = torch.from_numpy(ctx.denoise(raw, guides, dp)).cuda()
    ctx.tonemap(den.data_ptr(), W, H, 1, e, 2.2)
    out_path = sys.argv[7]
    den_path = out_path[:-4] + "_denoised.png" if out_path.lower().endswith(".png") else out_path + "_denoised.png"
    png.save_png(den_path, den.cpu().numpy()[..., :3], flipped=True)
    print("wrote", den_path, {k: float(dp[k]) for k in ("sigma_color", "sigma_normal", "sigma_plane")}, "ms", ctx.denoise_info()["ms_last"])
