"""What object motion costs (DESIGN.md section 2 "Object motion", docs/LOG.md).  usage (GPU box): python tools/rewind_time.py [--reps N]

The bench workload at its own size: the kitchen stand-in, 1920 x 1080, the guide planes of its camera in device buffers.  ms is the library's own ms_last (the
call's wall time with its launch and synchronisation), median and minimum over N calls after a warm-up: skh_rewind_guides with a table in which no instance
moved (every pixel is copied) and with one in which every instance moved (every surface pixel is transformed), out of place and in place; beside them
skh_set_instance_motion for the scene's table.  The yardstick: the 80 bytes per pixel a call cannot avoid -- 48 read (ids, position, normal), 32 written -- at the
copy rate skh_probe_memory measures on the same box in the same run (`over_floor` = measured / floor, temporal_time.py's figure), and the time of a device copy
that moves exactly those 80 bytes per pixel (a buffer of 40, read and written), which carries a launch of its own but not the call's host side.
Prints one JSON object."""
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

W, H = 1920, 1080
BYTES = 48 + 32


def main():
    from strelka_amd import capi, scene as S, scenes

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 15
    sc = scenes.kitchen_standin()
    arr = sc.arrays()
    ctx = capi.Context(0)
    ctx.set_scene(arr)
    ctx.resize(W, H)
    out = {"scene": "kitchen_standin", "width": W, "height": H, "pixels": W * H, "reps": reps, "instances": len(arr["instances"])}
    gbps, _ = ctx.probe_memory(0, 1 << 30, repeat=5)  # SKH_PROBE_COPY
    out["copy_gbps"] = round(gbps, 1)
    same_gbps, same_ms = ctx.probe_memory(0, (BYTES // 2) * W * H, repeat=5)
    out["copy_of_80_bytes_per_pixel"] = {"ms": round(same_ms, 4), "gbps": round(same_gbps, 1)}
    floor_ms = BYTES * W * H / (gbps * 1e9) * 1e3

    def stat(ms):
        s = {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4)}
        s.update(floor_bytes_per_pixel=BYTES, floor_ms=round(floor_ms, 4), over_floor=round(s["ms_min"] / floor_ms, 2), over_copy=round(s["ms_min"] / same_ms, 2))
        return s

    names = ("ids", "position", "normal")
    mask = sum(1 << S.AOV_PLANES.index(n) for n in names)
    guides = {n: ctx.buffer_alloc(16 * W * H) for n in names}
    ctx.render_aovs_device(S.aov_params(sc.getCamera(), W, H), mask, [guides.get(n) for n in S.AOV_PLANES])
    outs = [ctx.buffer_alloc(16 * W * H) for _ in range(2)]
    moved = arr["instances"].copy()
    moved["transform"][:, [3, 7, 11]] += np.array([0.01, 0.02, 0.03], np.float32)
    tables = {"no_instance_moved": S.instance_motion(arr["instances"], arr["instances"]), "every_instance_moved": S.instance_motion(arr["instances"], moved)}
    # (a light proxy whose transform is singular comes out MOVED | DROP; no surface pixel has its id)
    assert not tables["no_instance_moved"]["flags"].any() and (tables["every_instance_moved"]["flags"] & 1).all()
    ids = np.zeros((H, W, 4), np.uint32)
    ctx.buffer_download(guides["ids"], ids)
    out["surface_pixels"] = int(((ids[..., 3] == 1) | (ids[..., 3] == 2)).sum())
    for name, table in tables.items():
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.set_instance_motion(table)
            ms.append((time.perf_counter() - t0) * 1e3)
        out["set_instance_motion_" + name] = {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "bytes": int(table.nbytes)}
        for where, (po, no) in (("", outs), ("_in_place", (guides["position"], guides["normal"]))):
            if where and name == "every_instance_moved":
                continue  # (in place a moved table would move the planes again and again: the copy case times the aliasing)
            args = (W, H, guides["ids"], guides["position"], guides["normal"], po, no)
            ctx.rewind_guides_device(*args)
            ms = []
            for _ in range(reps):
                ctx.rewind_guides_device(*args)
                ms.append(ctx.rewind_info()["ms_last"])
            out["rewind_" + name + where] = stat(ms)
    for d in list(guides.values()) + outs:
        ctx.buffer_free(d)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
