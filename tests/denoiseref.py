"""The denoiser's definition (include/strelka_hip.h, "Denoiser") in numpy float64, one level at a time, with a per-pixel error bar for the
float32 evaluation that is a written-out count of roundings, as tests/hitref.py and tests/aovref.py do it.  u = 2^-24 is float32's unit roundoff.

The value.  For a surface pixel p and the level's input c:  out(p) = sum_q w(q) c(q) / sum_q w(q),  w(q) = h[dx] h[dy] exp(-min(a(q), 64)),
a = |c(q) - c(p)|^2 kc + |N(q) - N(p)|^2 kn + dot(N(p), P(q) - P(p))^2 kp over the taps that lie in the image and are surface pixels.  Here everything is float64
and kc, kn, kp are 1 / sigma^2 of the float32 sigmas.

The bar has two parts (plus, for a level that is not the first of a chain, what its input's own bar does: `ein` below).

  1. the sums and the division, with exact weights:  K u S,  S = sum w |c(q)| / sum w  (= |out| for colours of one sign).
     K = 51: the numerator's term w c(q) is one product (1) and goes through at most 24 of the 25 sequential additions (24, the first addition to 0 being exact);
     the denominator's w through 24 additions (24); the quotient (1); one more for the terms of second order in u.
  2. the weights:  2 sum_q w(q) dw(q) |c(q) - out| / sum w,  dw(q) = the relative error of tap q's weight: relative errors e(q) of the weights move the normalised
     sum by sum w e (c - out) / sum w to first order; the factor 2 covers the rest.  (2 max_q dw(q) max_q |c(q) - out| bounds this from above; the sum is kept as it
     is -- never wider --, because the largest dw belongs to taps across an edge, whose weight is e^-20 and less.)  dw(q) = expm1(da(q)) + 3.2 u:
       3.2 u   skh_libm's exp is within 1.1 ulp = 2.2 u of e^x (its stated bound, kept by tests/test_libm.py); the product with h[dx] h[dy] (itself exact) is one more
       da      the absolute error of a, which exp turns into a relative one:
               colour term tc   e_i = c(q)_i - c(p)_i (u each, so 2 u on its square), the square's rounding (1), two additions (2), the product with kc (1), and kc
                                itself = 1 / (sc sc), a product and a quotient (2): 8 u tc.  All terms are >= 0, so relative counts add.
               normal term tn   the same: 8 u tn
               plane term  tp   d = sum N_k g_k, g_k = P(q)_k - P(p)_k: per k the difference (u) and the product (u), and two additions whose partial sums are at
                                most D1 = sum |N_k g_k|: |error of d| <= 4 u D1 -- the cancellation is counted against D1, not against d.  Then
                                tp = d d kp: 2 |d| (4 u D1) kp + (4 u D1)^2 kp for d's error, and 4 u tp for the square (1), the product (1) and kp (2)
               the two additions of a: 2 u a
               An a of which both the float64 value and every float32 value within da lie above 64 is clamped on both sides: da = 0 there.  The clamp is
               continuous (and 1-Lipschitz), so nothing else changes at 64: no pixel is excluded.

Demodulation is one correctly rounded float32 division per channel: the reference does it in float32 too and gets the device's bits.  Remodulation is one float32
product of the last level's output: the bar is scaled by the factor and one u |result| is added.

A chain.  When the level's input on the device may differ from the reference's by up to ein(p) per channel (the previous level's bar), the output moves by at most
sum w ein(q) / sum w directly, and the colour term of a by at most kc sum_i (2 |e_i| E_i + E_i^2), E_i = ein(q)_i + ein(p)_i, which joins da; |c(q) - out| in
part 2 grows by ein(q)."""
import numpy as np

U = 2.0 ** -24
H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
K_SUMS = 51.0
EXP_AND_PRODUCT = 3.2 * U
KIND_SURFACE = (1, 2)
DEMODULATE, REMODULATE = 1, 2


def surface_mask(color, ids):
    """(h, w) bool: kind 1 or 2 and finite r, g, b"""
    kind = np.asarray(ids)[..., 3]
    return ((kind == 1) | (kind == 2)) & np.isfinite(np.asarray(color)[..., :3]).all(axis=-1)


def modulation(albedo, floor):
    """the definition's m = albedo > floor ? albedo : floor, float32 (a NaN albedo gives the floor)"""
    a = np.asarray(albedo, np.float32)[..., :3]
    with np.errstate(invalid="ignore"):
        return np.where(a > np.float32(floor), a, np.float32(floor)).astype(np.float32)


def inv_sq(sigma):
    """1 / sigma^2 in float64 of a float32 sigma; 0 for +inf"""
    s = float(np.float32(sigma))
    return 0.0 if np.isinf(s) else 1.0 / (s * s)


def level(c, valid, N, P, lvl, sigma_color, sigma_normal, sigma_plane, ein=None):
    """one level.  c (h, w, 3) float64, valid (h, w) bool, N, P (h, w, 3) -> (out (h, w, 3) float64, bar (h, w, 3)); rows of pixels that are not valid are 0."""
    c, N, P = (np.asarray(a, np.float64) for a in (c, N, P))
    h, w = valid.shape
    s = 1 << lvl
    kc = inv_sq(np.float32(sigma_color) * np.float32(2.0 ** -lvl))
    kn, kp = inv_sq(sigma_normal), inv_sq(sigma_plane)
    ein = np.zeros_like(c) if ein is None else np.asarray(ein, np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    sw = np.zeros((h, w))
    sc, sabs, sein = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    taps = []
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = yy + dy * s, xx + dx * s
                inb = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.where(inb, qy, yy), np.where(inb, qx, xx)
                take = inb & valid[qy, qx] & valid
                cq, Nq, Pq, eq = c[qy, qx], N[qy, qx], P[qy, qx], ein[qy, qx]
                e = cq - c
                tc = (e * e).sum(-1) * kc
                n = Nq - N
                tn = (n * n).sum(-1) * kn
                g = Pq - P
                d = (N * g).sum(-1)
                D1 = np.abs(N * g).sum(-1)
                tp = d * d * kp
                a = tc + tn + tp
                E = eq + ein
                da = (8 * U * (tc + tn) + kp * (8 * U * np.abs(d) * D1 + 16 * U * U * D1 * D1) + 4 * U * tp + 2 * U * a
                      + kc * (2 * np.abs(e) * E + E * E).sum(-1))
                da = np.where(a - da >= 64.0, 0.0, da)
                da = np.where(np.isfinite(da), da, 0.0)  # (an a that is NaN or inf is 64 on both sides)
                wq = H5[dx + 2] * H5[dy + 2] * np.exp(-np.where(a <= 64.0, a, 64.0))
                dw = np.expm1(da) + EXP_AND_PRODUCT
                wq = np.where(take, wq, 0.0)  # (float64 and finite inputs: selecting here is the same thing)
                cq = np.where(take[..., None], cq, 0.0)
                sw += wq
                sc += wq[..., None] * cq
                sabs += wq[..., None] * np.abs(cq)
                sein += wq[..., None] * np.where(take[..., None], eq, 0.0)
                taps.append((wq * np.where(take, dw, 0.0), cq, np.where(take[..., None], eq, 0.0)))
        den = np.where(valid, sw, 1.0)[..., None]
        out = sc / den
        wpart = np.zeros((h, w, 3))
        for wdw, cq, eq in taps:
            wpart += wdw[..., None] * (np.abs(cq - out) + eq)
        bar = K_SUMS * U * sabs / den + 2.0 * wpart / den + sein / den
    out = np.where(valid[..., None], out, 0.0)
    bar = np.where(valid[..., None], bar, 0.0)
    return out, bar


def denoise(color, ids, normal, position, albedo, params):
    """the whole call on float32 planes as the device gets them ((h, w, 4) each; albedo may be None when no flag is set) and an S.DENOISE_PARAMS record ->
    {"out": (h, w, 3) float64, "bar": (h, w, 3), "surface": (h, w) bool}.  Pixels outside `surface` and every alpha word are the input's bits: check() compares them so."""
    color = np.asarray(color, np.float32)
    valid = surface_mask(color, ids)
    flags = int(params["flags"])
    c32 = color[..., :3].copy()
    m = modulation(albedo, params["albedo_floor"]) if flags else None
    with np.errstate(all="ignore"):
        if flags & DEMODULATE:
            c32 = np.where(valid[..., None], c32 / m, c32).astype(np.float32)  # (one correctly rounded float32 division: the device's bits)
    c = np.where(valid[..., None], c32, 0.0).astype(np.float64)
    N, P = np.asarray(normal, np.float64)[..., :3], np.asarray(position, np.float64)[..., :3]
    bar = None
    for k in range(int(params["levels"])):
        c, bar = level(c, valid, N, P, int(params["first_level"]) + k, params["sigma_color"], params["sigma_normal"], params["sigma_plane"], ein=bar)
    if flags & REMODULATE:
        c = c * m
        bar = bar * m + U * np.abs(c)
        c, bar = np.where(valid[..., None], c, 0.0), np.where(valid[..., None], bar, 0.0)
    return {"out": c, "bar": bar, "surface": valid}


def params(width, height, first_level=0, levels=1, sigma_color=0.5, sigma_normal=0.3, sigma_plane=0.05, albedo_floor=0.05, flags=0):
    from strelka_amd import scene as S

    p = S.denoise_params(width, height, levels=levels, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_plane=sigma_plane, first_level=first_level,
                         albedo_floor=albedo_floor, demodulate=bool(flags & DEMODULATE), remodulate=bool(flags & REMODULATE))
    return p


def synthetic(width=67, height=45, seed=3, special=True):
    """synthetic planes for the filter, (h, w, 4) each: two planes that meet in a crease (at x = width / 2), a depth step of 0.5 with equal normals (the left plane's rows
    from 2/3 of the height on), a 0.9 / 0.1 checker albedo with a patch below the floor, uniform noise on a smooth irradiance; with `special` a band of kind 0, a band of
    kind 3, a band of kind 2, one NaN and one Inf colour, and alpha words of every sort (NaN patterns among them)."""
    rs = np.random.RandomState(seed)
    h, w = height, width
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    xc = w // 2
    left = x < xc
    N = np.zeros((h, w, 4), np.float32)
    P = np.zeros((h, w, 4), np.float32)
    N[..., :3] = np.where(left[..., None], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0])
    P[..., 0] = np.where(left, x * 0.1, xc * 0.1)
    P[..., 1] = np.where(left, 0.0, (x - xc) * 0.1)
    P[..., 2] = y * 0.1
    P[..., 1] += np.where(left & (y >= (2 * h) // 3), 0.5, 0.0)
    N[..., 3], P[..., 3] = 1.0, 1.0
    ids = np.zeros((h, w, 4), np.uint32)
    ids[..., 3] = 1
    A = np.ones((h, w, 4), np.float32)
    A[..., :3] = np.where((((x // 4) + (y // 4)) % 2 == 0)[..., None], 0.9, 0.1)
    if h > 8 and w > 8:
        A[2:5, 2:6, :3] = [0.0, 0.01, 0.2]  # (below, below and above the floor)
    irr = 0.6 + 0.3 * np.sin(x * 0.11) * np.cos(y * 0.07)
    C = np.zeros((h, w, 4), np.float32)
    C[..., :3] = A[..., :3] * (irr[..., None] + rs.uniform(-0.4, 0.4, (h, w, 3)))
    C[..., 3] = rs.uniform(0.0, 1.0, (h, w))
    if special and h >= 40 and w >= 64:
        C[..., 3].view(np.uint32)[0, :8] = [0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000, 0xDEADBEEF, 0x7FBFFFFF]
        for (y0, y1, x0, x1, kind) in ((10, 12, 5, 26, 0), (14, 16, 40, 61, 3), (20, 23, 0, w, 2)):
            ids[y0:y1, x0:x1, 3] = kind
            if kind == 0:
                ids[y0:y1, x0:x1, :3] = 0xFFFFFFFF
                N[y0:y1, x0:x1], P[y0:y1, x0:x1], A[y0:y1, x0:x1] = 0.0, 0.0, 0.0
                C[y0:y1, x0:x1, :3] = 0.0
            if kind == 3:
                N[y0:y1, x0:x1] = 0.0
                A[y0:y1, x0:x1] = 1.0
                C[y0:y1, x0:x1, :3] = 40.0
            if kind == 2:
                # a band whose normals turn along x while its points climb a ramp: N(q) differs from N(p) by little, and dot(N(p), g) from dot(N(q), g) by a lot
                phi = 0.0004 * x[y0:y1, x0:x1] ** 2
                N[y0:y1, x0:x1, 0], N[y0:y1, x0:x1, 1], N[y0:y1, x0:x1, 2] = np.sin(phi), np.cos(phi), 0.0
                P[y0:y1, x0:x1, 0], P[y0:y1, x0:x1, 1] = 0.1 * x[y0:y1, x0:x1], 0.03 * x[y0:y1, x0:x1]
        C[5, 7, 0] = np.nan
        C[35, 50, 1] = np.inf
    return {"color": C, "ids": ids, "normal": N, "position": P, "albedo": A}


def check(got, color, ref):
    """`got`: the device's (h, w, 4) float32 image for the input `color`.  Asserts the bit-exact parts -- alpha everywhere, every word of a pixel that is no surface
    pixel -- and returns the worst |got - out| / bar over ALL surface pixels and channels (0 where both are 0): the caller asserts <= 1."""
    got, color = np.asarray(got, np.float32), np.asarray(color, np.float32)
    assert got.shape == color.shape
    surf = ref["surface"]
    assert np.array_equal(got[..., 3].view(np.uint32), color[..., 3].view(np.uint32)), "an alpha word changed"
    assert np.array_equal(got[~surf].view(np.uint32), color[~surf].view(np.uint32)), "a pixel that is no surface pixel changed"
    assert np.isfinite(got[surf][:, :3]).all(), "a non-finite value on a surface pixel"
    err = np.abs(got[..., :3].astype(np.float64) - ref["out"])[surf]
    bar = ref["bar"][surf]
    ratio = np.where(err == 0.0, 0.0, err / np.where(bar > 0.0, bar, np.finfo(np.float64).tiny))
    return float(ratio.max()) if ratio.size else 0.0
