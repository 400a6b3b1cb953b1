"""What variance guidance costs (DESIGN.md section 2 "Variance guidance", docs/LOG.md).  usage (GPU box): python tools/variance_time.py [--reps N] [--parent-lib PATH]

The bench workload at its own size, as tools/temporal_time.py sets it up: the kitchen stand-in, 1920 x 1080, two cameras a step of the interactive orbit apart, a
raw 1-spp image and the guide planes of each in device buffers.  ms is the library's own ms_last (the call's wall time with its launch and synchronisation),
median and minimum over N calls after a warm-up, the calls of a pair ALTERNATING in one loop so that both see the same clocks:

  skh_moments (with previous moments)             against a device copy of the 176 bytes per pixel it must move (96 read + 64 gathered + 16 written):
                                                  skh_probe_memory's stream copy rate on the same box; `over_floor` = measured / floor
  skh_denoise_variance, five levels, all flags    against skh_denoise, five levels, both flags, on the same planes -- of this library, and with --parent-lib also of
                                                  a second library (the parent commit's build) loaded beside it, on the same device buffers

Prints one JSON object."""
import copy
import ctypes as C
import json
import math
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H = 1920, 1080
MOMENTS_BYTES = 96 + 64 + 16


def main():
    from strelka_amd import capi, scene as S, scenes

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 15
    parent_path = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
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
    nbytes = 16 * W * H
    frames = []
    for k in range(2):
        cam = camera(k)
        f = {"aov": S.aov_params(cam, W, H), "image": ctx.buffer_alloc(nbytes), "guides": {n: ctx.buffer_alloc(nbytes) for n in names}}
        f["planes"] = [f["guides"].get(n) for n in S.AOV_PLANES]
        ctx.render_aovs_device(f["aov"], mask, f["planes"])
        ctx.render_subframe(S.frame_params(cam, W, H, subframe_index=k, spp_total=64, max_depth=4, enable_accumulation=0), f["image"])
        frames.append(f)
    a, b = frames
    ga, gb = a["guides"], b["guides"]
    d_out, d_motion, d_filtered = (ctx.buffer_alloc(nbytes) for _ in range(3))
    history = [ctx.buffer_alloc(nbytes) for _ in range(2)]
    moments = [ctx.buffer_alloc(nbytes) for _ in range(2)]
    p0 = S.temporal_params(W, H, scene=arr)
    p1 = S.temporal_params(W, H, a["aov"], scene=arr)
    ctx.temporal_device(p0, a["image"], ga["ids"], ga["normal"], ga["position"], ga["albedo"], None, None, None, None, d_out, history[0], None)
    ctx.moments_device(p0, a["image"], ga["ids"], ga["position"], ga["albedo"], None, None, moments[0])
    ctx.temporal_device(p1, b["image"], gb["ids"], gb["normal"], gb["position"], gb["albedo"], history[0], ga["ids"], ga["normal"], ga["position"], d_out, history[1], d_motion)

    # skh_moments
    margs = (p1, b["image"], gb["ids"], gb["position"], gb["albedo"], d_motion, moments[0], moments[1])
    ctx.moments_device(*margs)
    ms = []
    for _ in range(reps):
        ctx.moments_device(*margs)
        ms.append(ctx.moments_info()["ms_last"])
    out["moments"] = stat(ms, MOMENTS_BYTES)
    ms = []
    for _ in range(reps):
        ctx.moments_device(p0, b["image"], gb["ids"], gb["position"], gb["albedo"], None, None, moments[1])
        ms.append(ctx.moments_info()["ms_last"])
    out["moments_no_previous_frame"] = stat(ms, 64 + 16)
    ctx.moments_device(*margs)

    # the two filters on the blended image, alternating
    host = np.zeros((H, W, 4), np.float32)
    ctx.buffer_download(d_out, host)
    guides_host = {}
    for n in ("ids", "albedo"):
        guides_host[n] = np.zeros((H, W, 4), np.uint32 if n == "ids" else np.float32)
        ctx.buffer_download(gb[n], guides_host[n])
    dp = S.denoise_params(W, H, levels=5, scene=arr, image=host, guides=guides_host)
    vp = S.vdenoise_params(W, H, levels=5, scene=arr, image=host, guides=guides_host)
    out["params"] = {"sigma_color": float(dp["sigma_color"]), "sigma_luminance": float(vp["sigma_luminance"]), "epsilon": float(vp["epsilon"]),
                     "min_history": float(vp["min_history"])}
    plain = (dp, d_out, gb["ids"], gb["normal"], gb["position"], gb["albedo"], d_filtered)
    guided = (vp, d_out, gb["ids"], gb["normal"], gb["position"], gb["albedo"], moments[1], d_filtered, None)
    parent = None
    if parent_path:
        lib = C.CDLL(parent_path)
        for fn, n in (("skh_create", 2), ("skh_denoise", 8), ("skh_get_denoise_info", 2), ("skh_destroy", 1)):
            getattr(lib, fn).restype = C.c_int
        h = C.c_void_p()
        assert lib.skh_create(0, C.byref(h)) == 0
        info = np.zeros((), capi.DENOISE_INFO)

        def parent():
            assert lib.skh_denoise(h, dp.ctypes.data_as(C.c_void_p), *[C.c_void_p(getattr(x, "value", x)) for x in plain[1:]]) == 0
            assert lib.skh_get_denoise_info(h, info.ctypes.data_as(C.c_void_p)) == 0
            return float(info["ms_last"])

        parent()
    ctx.denoise_device(*plain)
    ctx.denoise_variance_device(*guided)
    t = {"denoise": [], "denoise_variance": [], "denoise_parent_library": []}
    for _ in range(reps):
        ctx.denoise_device(*plain)
        t["denoise"].append(ctx.denoise_info()["ms_last"])
        ctx.denoise_variance_device(*guided)
        t["denoise_variance"].append(ctx.vdenoise_info()["ms_last"])
        if parent:
            t["denoise_parent_library"].append(parent())
    for k, v in t.items():
        if v:
            out[k + "_5_levels"] = stat(v)
    out["guided_over_plain"] = round(out["denoise_variance_5_levels"]["ms_min"] / out["denoise_5_levels"]["ms_min"], 3)
    # the share of the pixels that take the 7 x 7 estimate, and the filter without it
    nm = np.zeros((H, W, 4), np.float32)
    ctx.buffer_download(moments[1], nm)
    kind = guides_host["ids"][..., 3]
    surf = (kind == 1) | (kind == 2)
    out["estimate_share_of_surface_pixels"] = round(float((nm[..., 3][surf] < float(vp["min_history"])).mean()), 4)
    vq = np.array(vp)
    vq["flags"] = 3
    ms = []
    for _ in range(reps):
        ctx.denoise_variance_device(vq, *guided[1:])
        ms.append(ctx.vdenoise_info()["ms_last"])
    out["denoise_variance_5_levels_without_estimate"] = stat(ms)
    if parent:
        lib.skh_destroy(h)
    for f in frames:
        for d in [f["image"]] + list(f["guides"].values()):
            ctx.buffer_free(d)
    for d in [d_out, d_motion, d_filtered] + history + moments:
        ctx.buffer_free(d)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
