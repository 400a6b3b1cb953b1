"""What history rectification costs (DESIGN.md section 2 "History rectification", docs/LOG.md).  usage (GPU box): python tools/rectify_time.py [--reps N]

The bench workload at its own size: the kitchen stand-in, 1920 x 1080, two cameras a step of the interactive orbit (0.25 degrees) apart, a raw 1-spp image and
the guide planes of each in device buffers, a long and a fast history of the first frame and what skh_temporal makes of them in the second.  ms is the library's
own ms_last (the call's wall time with its launch and synchronisation), median and minimum over N calls after a warm-up: skh_rectify at each radius, with and
without the info plane; beside them, in the same run, the fast history's skh_temporal call and one 1-spp sub-frame of the same scene -- a rectified HipRender
call pays one more skh_temporal and one skh_rectify.  The yardstick: the bytes a call must move once -- per pixel 80 read (image, ids, albedo, history, fast),
32 written (image, history) or 48 with the info plane -- at the copy rate skh_probe_memory measures on the same box; `over_floor` = measured / floor.
Prints one JSON object."""
import copy
import json
import math
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H = 1920, 1080
READ_BYTES, WRITE_BYTES, INFO_BYTES = 80, 32, 16


def main():
    from strelka_amd import capi, scene as S, scenes

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 15
    sc = scenes.kitchen_standin()
    arr = sc.arrays()
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    ctx.resize(W, H)
    out = {"scene": "kitchen_standin", "width": W, "height": H, "pixels": W * H, "reps": reps}
    gbps, _ = ctx.probe_memory(0, 1 << 30, repeat=5)  # SKH_PROBE_COPY
    out["copy_gbps"] = round(gbps, 1)

    def stat(ms, floor_bytes=None):
        s = {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4)}
        if floor_bytes:
            floor_ms = floor_bytes * W * H / (gbps * 1e9) * 1e3
            s.update(floor_bytes_per_pixel=floor_bytes, floor_ms=round(floor_ms, 4), over_floor=round(s["ms_min"] / floor_ms, 2))
        return s

    cam0 = copy.deepcopy(sc.getCamera())
    eye0 = np.array(cam0.position, np.float64)
    target = eye0 - np.array(cam0.rotation[2, :3], np.float64) * 3.0

    def camera(k):
        cam, a, r = copy.deepcopy(cam0), math.radians(0.25 * k), eye0 - target
        cam.lookAt(tuple(target + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])), tuple(target))
        return cam

    names = capi.DENOISE_GUIDES
    mask = sum(1 << S.AOV_PLANES.index(n) for n in names)
    frames = []
    for k in range(2):
        cam = camera(k)
        f = {"aov": S.aov_params(cam, W, H), "image": ctx.buffer_alloc(16 * W * H), "guides": {n: ctx.buffer_alloc(16 * W * H) for n in names}}
        f["frame"] = S.frame_params(cam, W, H, subframe_index=k, spp_total=64, max_depth=4, enable_accumulation=0)
        ctx.render_aovs_device(f["aov"], mask, [f["guides"].get(n) for n in S.AOV_PLANES])
        ctx.render_subframe(f["frame"], f["image"])
        frames.append(f)
    a, b = frames
    ms = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.render_subframe(b["frame"], b["image"])
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["subframe_1spp"] = stat(ms)
    # the two histories of the first frame, and the second frame's skh_temporal calls
    bufs = {n: ctx.buffer_alloc(16 * W * H) for n in ("long0", "fast0", "scratch", "image", "long1", "fast1", "out", "history_out", "info")}
    long_p = lambda aov: S.temporal_params(W, H, aov, scene=arr)
    fast_p = lambda aov: S.temporal_params(W, H, aov, max_history=S.RECTIFY_FAST_HISTORY, scene=arr)
    g, h = a["guides"], b["guides"]
    for p, hist in ((long_p(None), "long0"), (fast_p(None), "fast0")):
        ctx.temporal_device(p, a["image"], g["ids"], g["normal"], g["position"], g["albedo"], None, None, None, None, bufs["scratch"], bufs[hist], None)
    ctx.temporal_device(long_p(a["aov"]), b["image"], h["ids"], h["normal"], h["position"], h["albedo"], bufs["long0"], g["ids"], g["normal"], g["position"],
                        bufs["image"], bufs["long1"], None)
    fast_args = (fast_p(a["aov"]), b["image"], h["ids"], h["normal"], h["position"], h["albedo"], bufs["fast0"], g["ids"], g["normal"], g["position"],
                 bufs["scratch"], bufs["fast1"], None)
    ctx.temporal_device(*fast_args)
    ms = []
    for _ in range(reps):
        ctx.temporal_device(*fast_args)
        ms.append(ctx.temporal_info()["ms_last"])
    out["temporal_fast_history"] = stat(ms, 80 + 64 + 32)
    out["params"] = {"k": S.RECTIFY_K, "fast_history": S.RECTIFY_FAST_HISTORY, "shorten": S.RECTIFY_SHORTEN_DEFAULT}
    for radius in (1, 2, 3):
        p = S.rectify_params(W, H, radius=radius)
        for info in (False, True):
            args = (p, bufs["image"], h["ids"], h["albedo"], bufs["long1"], bufs["fast1"], bufs["out"], bufs["history_out"], bufs["info"] if info else None)
            ctx.rectify_device(*args)
            ms = []
            for _ in range(reps):
                ctx.rectify_device(*args)
                ms.append(ctx.rectify_info()["ms_last"])
            out[f"rectify_radius_{radius}" + ("_with_info" if info else "")] = stat(ms, READ_BYTES + WRITE_BYTES + (INFO_BYTES if info else 0))
    plane = np.zeros((H, W, 4), np.float32)
    ctx.buffer_download(bufs["info"], plane)
    out["radius_3_pixels"] = {"rectified": int((plane[..., 1] > 0).sum()), "clamped": int((plane[..., 0] != 0).sum())}
    for f in frames:
        for d in [f["image"]] + list(f["guides"].values()):
            ctx.buffer_free(d)
    for d in bufs.values():
        ctx.buffer_free(d)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
