"""What the denoiser costs (DESIGN.md section 2 "Denoiser", docs/LOG.md).  usage (GPU box): python tools/denoise_time.py [--reps N]

The bench workload at its own size: the kitchen stand-in, 1920 x 1080, a 1-spp image and its guide planes in device buffers.  ms is the library's own ms_last (the
call's wall time with its synchronisation), median and minimum over N calls after a warm-up: the whole call (five levels, both flags), each level alone (a one-level call is the pack pass and one level launch; the pack
pass is estimated as levels 0 and 1 alone less the two-level call, and taken off: `level_ms_estimate`), the guide pass
(skh_render_aovs, four planes), and beside them one 1-spp sub-frame of the same scene.  The yardstick per level: the bytes a level cannot avoid -- 64 per
pixel: a colour record in, a guide record in, a colour record out -- at the copy rate skh_probe_memory measures on the same box; `over_floor` = measured /
floor.  Prints one JSON object."""
import json
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H = 1920, 1080
FLOOR_BYTES = 64


def main():
    from strelka_amd import capi, scene as S, scenes

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
    sc = scenes.kitchen_standin()
    arr = sc.arrays()
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    ctx.resize(W, H)
    out = {"scene": "kitchen_standin", "width": W, "height": H, "pixels": W * H, "reps": reps}
    gbps, _ = ctx.probe_memory(0, 1 << 30, repeat=5)
    floor_ms = FLOOR_BYTES * W * H / (gbps * 1e9) * 1e3
    out["copy_gbps"], out["level_floor_ms"], out["level_floor_bytes_per_pixel"] = round(gbps, 1), round(floor_ms, 4), FLOOR_BYTES

    def stat(ms):
        return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4)}

    # one 1-spp sub-frame into a device image
    d_image, d_out = ctx.buffer_alloc(16 * W * H), ctx.buffer_alloc(16 * W * H)
    p = S.frame_params(sc.getCamera(), W, H, subframe_index=0, spp_total=1, max_depth=4)
    ctx.render_subframe(p, d_image)
    ms = []
    import time
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.render_subframe(p, d_image)
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["subframe_1spp"] = stat(ms)
    # the guide pass
    ap = S.aov_params(sc.getCamera(), W, H)
    bufs = {n: ctx.buffer_alloc(16 * W * H) for n in capi.DENOISE_GUIDES}
    planes = [bufs.get(n) for n in S.AOV_PLANES]
    mask = sum(1 << S.AOV_PLANES.index(n) for n in capi.DENOISE_GUIDES)
    ctx.render_aovs_device(ap, mask, planes)
    ms = []
    for _ in range(reps):
        ctx.render_aovs_device(ap, mask, planes)
        ms.append(ctx.aov_info()["ms_last"])
    out["guide_pass"] = stat(ms)
    # the filter
    noisy = np.zeros((H, W, 4), np.float32)
    ctx.buffer_download(d_image, noisy)
    guides = {n: np.zeros((H, W, 4), np.uint32 if n == "ids" else np.float32) for n in ("ids", "albedo")}
    for n in guides:
        ctx.buffer_download(bufs[n], guides[n])
    base = S.denoise_params(W, H, scene=arr, image=noisy, guides=guides)
    out["params"] = {k: float(base[k]) for k in ("sigma_color", "sigma_normal", "sigma_plane", "albedo_floor")}
    out["surface_pixels"] = int((((guides["ids"][..., 3] == 1) | (guides["ids"][..., 3] == 2)) & np.isfinite(noisy[..., :3]).all(-1)).sum())

    def run(params):
        args = (params, d_image, bufs["ids"], bufs["normal"], bufs["position"], bufs["albedo"], d_out)
        ctx.denoise_device(*args)
        ms = []
        for _ in range(reps):
            ctx.denoise_device(*args)
            ms.append(ctx.denoise_info()["ms_last"])
        return stat(ms)

    out["five_levels"] = run(base)
    one = {}
    for lvl in range(5):
        q = np.array(base)
        q["first_level"], q["levels"] = lvl, 1
        one[lvl] = run(q)
    # a one-level call is the pack pass and one level launch; two levels less one level is one level launch alone
    two = np.array(base)
    two["first_level"], two["levels"] = 0, 2
    t2 = run(two)
    pack = max(0.0, one[0]["ms_min"] + one[1]["ms_min"] - t2["ms_min"])
    out["pack_pass_ms_estimate"] = round(pack, 4)
    out["levels"] = {}
    for lvl in range(5):
        level_ms = max(0.0, one[lvl]["ms_min"] - pack)
        out["levels"][str(lvl)] = dict(one[lvl], level_ms_estimate=round(level_ms, 4), over_floor=round(level_ms / floor_ms, 2))
    out["scratch_bytes"] = ctx.denoise_info()["scratch_bytes"]
    for b in list(bufs.values()) + [d_image, d_out]:
        ctx.buffer_free(b)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
