"""What a first-hit AOV call costs (DESIGN.md section 2 "First-hit AOVs", docs/LOG.md).  usage (GPU box): python tools/aov_time.py [--reps N]

The bench workload at its own size: the kitchen stand-in, 1920 x 1080.  Per call of skh_render_aovs into device buffers allocated once: ms (the library's own
ms_last: the call's wall time with its synchronisation) for planes ids | hit alone and for all seven planes, through the pixel centres and for sample 0; the median
and the minimum over N calls after a warm-up.  Beside them the yardstick: ms_trace_closest (option timing) of ONE 1-spp, depth-1 sub-frame of the same scene -- one
closest-hit launch over the same 2.07 M camera rays.  Prints one JSON object."""
import json
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H = 1920, 1080


def main():
    from strelka_amd import capi, scene as S, scenes

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    sc = scenes.kitchen_standin()
    ctx = capi.Context(0)
    ctx.set_scene(sc.arrays())
    ctx.resize(W, H)
    ctx.set_option("timing", 1)
    out = {"scene": "kitchen_standin", "width": W, "height": H, "rays_per_call": W * H}
    # the yardstick: one closest-hit launch of a 1-spp, depth-1 sub-frame
    p = S.frame_params(sc.getCamera(), W, H, subframe_index=0, spp_total=1, max_depth=1)
    ctx.render_subframe(p)  # warm-up
    ys = []
    for _ in range(reps):
        ctx.reset_stats()
        ctx.render_subframe(p)
        ctx.synchronize()
        st = ctx.stats()
        ys.append(st["ms_trace_closest"])
        launches = st["launches_trace_closest"]
    out["subframe_1spp_depth1"] = {"ms_trace_closest_median": round(statistics.median(ys), 4), "ms_trace_closest_min": round(min(ys), 4), "launches_trace_closest": launches}
    bufs = [ctx.buffer_alloc(16 * W * H) for _ in S.AOV_PLANES]
    for mode, sample in (("centre", None), ("sample0", 0)):
        ap = S.aov_params(sc.getCamera(), W, H, sample_index=sample, spp_total=64)
        for label, mask in (("ids_hit", 0b11), ("all_seven", (1 << len(S.AOV_PLANES)) - 1)):
            ctx.render_aovs_device(ap, mask, bufs)  # warm-up
            ms = []
            for _ in range(reps):
                ctx.render_aovs_device(ap, mask, bufs)
                ms.append(ctx.aov_info()["ms_last"])
            out[f"{mode}_{label}"] = {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "plane_bytes": ctx.aov_info()["bytes_last"]}
    ids = np.zeros((H, W, 4), np.uint32)
    ctx.buffer_download(bufs[0], ids)
    out["kinds"] = {str(k): int((ids[..., 3] == k).sum()) for k in range(4)}
    for b in bufs:
        ctx.buffer_free(b)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
