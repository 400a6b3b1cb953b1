"""Adaptive sampling restated ("Adaptive sampling"; strelka_amd/csrc/skh_adapt.h): numpy only.

An OBSERVATION of a pixel is what one launch hands to the accumulator (radiance sum / samples of the launch).  y = 0.2126 t.x + 0.7152 t.y + 0.0722 t.z with
t = c / (c + 1), c = observation * exposure; products and sums rounded one by one, left to right.  Welford per pixel: n += 1; d = y - mean; mean += d / n;
M2 += d * (y - mean).  A check happens at n >= min_samples with (n - min_samples) % interval == 0: v = M2 / n; e2 = v / n; ref = max(mean, dark_level);
q = e2 / (ref * ref); Q = max q over the tile's valid pixels; the tile freezes iff Q <= threshold * threshold (false for a NaN); frozen tiles never thaw.

`dtype` np.float32 is the device's arithmetic, operation for operation; np.float64 is the same text in double (the observations stay the float32 values they are)."""
import numpy as np

F = np.float32


def luma(obs, exposure, dtype=F):
    """(..., 3) observations -> (...) LDR luminance"""
    o, e = np.asarray(obs, F).astype(dtype), np.asarray(exposure, F).astype(dtype)
    c = o * e
    t = c / (c + dtype(1.0))
    return (dtype(0.2126) * t[..., 0] + dtype(0.7152) * t[..., 1]) + dtype(0.0722) * t[..., 2]


def fold(state, y):
    """one Welford step on state = [n, mean, M2] (arrays of y's shape and dtype), in place"""
    n, mean, m2 = state
    n += y.dtype.type(1.0)
    d = y - mean
    mean += d / n
    m2 += d * (y - mean)


def welford(ys, dtype=F):
    """ys (k, ...) -> (n, mean, M2) after the k observations in order"""
    ys = np.asarray(ys).astype(dtype)
    st = [np.zeros(ys.shape[1:], dtype) for _ in range(3)]
    for y in ys:
        fold(st, y)
    return st


def pixel_q(n, mean, m2, dark_level):
    dt = mean.dtype.type
    v = m2 / n
    e2 = v / n
    ref = np.maximum(mean, dt(dark_level))
    return e2 / (ref * ref)


def is_check(n, min_samples, interval):
    return n >= min_samples and (n - min_samples) % interval == 0


def tile_grid(width, height, tile):
    """the default tile list: row-major (x0, y0) origins"""
    return [(x, y) for y in range(0, height, tile) for x in range(0, width, tile)]


def schedule(obs, exposure, tile, threshold, dark_level, min_samples, interval, tiles=None, dtype=F):
    """The whole freeze schedule over obs (launches, H, W, 3): -> dict
         counts  per tile of `tiles` (default: the whole image's grid), the observations it received (its count when it froze, else all launches)
         state   (H, W, 4) {n, mean, M2, q at the tile's last check} in `dtype`; 0 outside `tiles`
         Q       per tile, at its last check (0 before the first)
         frozen  per tile, whether it froze (a tile may freeze at the very last launch: its count is then all launches as well)
         checks  the number of checks that ran (none once every tile is frozen)"""
    obs = np.asarray(obs, F)
    L, H, W = obs.shape[:3]
    tiles = tile_grid(W, H, tile) if tiles is None else [tuple(int(v) for v in t) for t in tiles]
    thr2 = dtype(F(threshold) * F(threshold))  # (the product is taken in float32 on the device)
    state = np.zeros((H, W, 4), dtype)
    counts, Q = [0] * len(tiles), [dtype(0.0)] * len(tiles)
    frozen = [False] * len(tiles)
    checks = 0
    ys = luma(obs, exposure, dtype)
    for k in range(L):
        if all(frozen):
            break
        n = k + 1
        for t, (x0, y0) in enumerate(tiles):
            if frozen[t]:
                continue
            sl = (slice(y0, min(H, y0 + tile)), slice(x0, min(W, x0 + tile)))
            st = [state[sl + (j,)] for j in range(3)]
            fold(st, ys[k][sl])
            counts[t] = n
        if not is_check(n, min_samples, interval):
            continue
        checks += 1
        for t, (x0, y0) in enumerate(tiles):
            if frozen[t]:
                continue
            sl = (slice(y0, min(H, y0 + tile)), slice(x0, min(W, x0 + tile)))
            if state[sl].size == 0:
                frozen[t] = True  # (a tile without a pixel inside the image: Q = 0)
                continue
            with np.errstate(all="ignore"):
                q = pixel_q(state[sl + (0,)], state[sl + (1,)], state[sl + (2,)], dark_level)
            state[sl + (3,)] = q
            Q[t] = q.max()  # (numpy's max keeps a NaN, as the device's does)
            frozen[t] = bool(Q[t] <= thr2)
    return {"counts": counts, "state": state, "Q": Q, "frozen": frozen, "checks": checks, "tiles": tiles}


def count_map(res, width, height, tile):
    """per-pixel observation counts of a schedule() result"""
    m = np.zeros((height, width), np.int64)
    for (x0, y0), n in zip(res["tiles"], res["counts"]):
        m[y0:y0 + tile, x0:x0 + tile] = n
    return m
