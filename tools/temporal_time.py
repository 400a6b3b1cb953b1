"""What temporal accumulation costs (DESIGN.md section 2 "Temporal accumulation", docs/LOG.md).  usage (GPU box): python tools/temporal_time.py [--reps N]

The bench workload at its own size: the kitchen stand-in, 1920 x 1080, two cameras a step of the interactive orbit (0.25 degrees) apart, a raw 1-spp image and
the guide planes of each in device buffers, the first frame's history from a call without a previous frame.  ms is the library's own ms_last (the call's wall
time with its launch and synchronisation), median and minimum over N calls after a warm-up: skh_temporal with a previous frame, with and without the motion
plane, and without a previous frame; beside them, in the same run, the guide pass (skh_render_aovs, four planes) and one 1-spp sub-frame of the same scene --
what a moving HipRender call is made of.  The yardstick: the bytes a call cannot avoid -- per pixel 80 of the current planes (colour, ids, normal, position,
albedo), 64 of the previous planes counted once (history, ids, normal, position), 32 written (image, history) or 48 with the motion plane -- at the copy rate
skh_probe_memory measures on the same box; `over_floor` = measured / floor.  Prints one JSON object."""
import copy
import json
import math
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H = 1920, 1080
READ_BYTES, WRITE_BYTES, MOTION_BYTES = 80 + 64, 32, 16


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
        f["planes"] = [f["guides"].get(n) for n in S.AOV_PLANES]
        ctx.render_aovs_device(f["aov"], mask, f["planes"])
        ctx.render_subframe(f["frame"], f["image"])
        frames.append(f)
    a, b = frames
    # one raw 1-spp sub-frame and the guide pass: the rest of a moving call
    ms = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.render_subframe(b["frame"], b["image"])
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["subframe_1spp"] = stat(ms)
    ms = []
    for _ in range(reps):
        ctx.render_aovs_device(b["aov"], mask, b["planes"])
        ms.append(ctx.aov_info()["ms_last"])
    out["guide_pass"] = stat(ms)
    # the pass
    d_out, d_motion = ctx.buffer_alloc(16 * W * H), ctx.buffer_alloc(16 * W * H)
    history = [ctx.buffer_alloc(16 * W * H) for _ in range(2)]
    p0 = S.temporal_params(W, H, scene=arr)
    p1 = S.temporal_params(W, H, a["aov"], scene=arr)
    out["params"] = {k: float(p1[k]) for k in ("normal_min", "plane_tolerance", "max_history", "albedo_floor")}
    g = a["guides"]
    ctx.temporal_device(p0, a["image"], g["ids"], g["normal"], g["position"], g["albedo"], None, None, None, None, d_out, history[0], None)

    def run(params, prev, motion):
        h = b["guides"]
        args = (params, b["image"], h["ids"], h["normal"], h["position"], h["albedo"]) + ((history[0], g["ids"], g["normal"], g["position"]) if prev else (None,) * 4) + (
            d_out, history[1], d_motion if motion else None)
        ctx.temporal_device(*args)
        ms = []
        for _ in range(reps):
            ctx.temporal_device(*args)
            ms.append(ctx.temporal_info()["ms_last"])
        return ms

    out["temporal"] = stat(run(p1, True, False), READ_BYTES + WRITE_BYTES)
    out["temporal_with_motion"] = stat(run(p1, True, True), READ_BYTES + WRITE_BYTES + MOTION_BYTES)
    out["temporal_no_previous_frame"] = stat(run(p0, False, False), 80 + WRITE_BYTES)
    mv = np.zeros((H, W, 4), np.float32)
    ctx.buffer_download(d_motion, mv)
    m = mv[..., 3]
    out["tap_masks"] = {"surface_or_projecting": int((mv[..., :3] != 0).any(-1).sum()), "all_four": int((m == 15).sum()), "some": int(((m > 0) & (m < 15)).sum())}
    for f in frames:
        for d in [f["image"]] + list(f["guides"].values()):
            ctx.buffer_free(d)
    for d in [d_out, d_motion] + history:
        ctx.buffer_free(d)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
