"""Variance guidance's definition (include/strelka_hip.h, "Variance guidance") in numpy.  u = 2^-24 is float32's unit roundoff; the counts of
roundings are written out as tests/denoiseref.py and tests/temporalref.py do it, and both are imported, neither changed.

moments32    skh_moments restated operation by operation in float32: + - x /, floor, compare and select, which numpy rounds as IEEE 754 says.  The device must give
             these bits.

moments64    the same in float64 on the same float32 planes, with a per-pixel bar.
  decisions  clip.w > 0, the range test and the two floors are temporalref.reproject64's, with its bars (ew, efx); a pixel whose margin lies inside the bar is
             AMBIGUOUS and compared with neither branch.  The mask word, the finiteness of the previous record and nm >= 1 read input words: no margin.  A pixel
             whose mask is 0 takes the branch without history whatever it projects to: never ambiguous.
  the value  l = lum(c): three products and two additions, five roundings counted against L = sum |coef c|: el = 5 u L.  l l: 2 |l| el + el^2 + u l l.
             m1, m2, nh as reproject64's h and nh (9 u S with exact weights; the weights' errors 2 sum ew_k |x_k - m| / sw);  nm' as its n'.
             mu' = m + (x - m) alpha: em + alpha ex + alpha |x - m| (en / nm' + 3 u) + 2 u (|m| + alpha |x - m|)   (x = l or l l; the difference, the product and
             alpha's quotient 3 u; the sum u, one spare, counted against the two terms).
             v = mu2' - mu1' mu1': e2 + 2 |mu1'| e1 + e1^2 + 2 u (|mu2'| + mu1'^2) -- the product's and the difference's roundings are ABSOLUTE, counted against
             mu2' + mu1'^2, not against the difference, which cancels.  The clamp at 0 is 1-Lipschitz: no pixel is excluded for it.

estimate64   the 7 x 7 estimate of skh_denoise_variance's input variance, float64 with a bar in denoiseref.level's style: the weight is exp alone (2.2 u, no product
             with h), a = tn + tp has one addition; K = 99 for the 49 taps (a product, 48 additions above and 48 below, the quotient, one spare);
             v = e2 - e1 e1 as above; k = min_history / max(nm, 1) is one quotient, v k one product: 3 u v k with the spare.

level64      one level, float64 with bars.  Colour: denoiseref.level's two parts with the colour term of a replaced by
               tl = |lum(c(q)) - lum(c(p))| kl: each lum 5 u L; the difference u; kl = 1 / (sigma sqrt(vbar) + epsilon) has the relative error of the two 3 x 3 sums
               (a product and up to 8 additions each, the quotient: 19 u), halved by the root (9.5 u), plus the root, the product, the sum and the quotient (4 u):
               13.5 u -- all terms are >= 0, so relative counts add; the product with kl one more:  dtl = kl (5 u (L(q) + L(p))) + 15.5 u tl.
             Variance: v_out = sum w^2 v / (sum w)^2.  With exact weights 53 u sum w^2 v / sw^2 (w w, its product with v, 24 additions, 24 below, sw sw, the
             quotient, one spare: "a product more per term").  Relative errors e(q) of the weights move it by 2 sum w e (w v(q) - v_out sw) / sw^2 to first order;
             doubled for the rest as in denoiseref.
             Underflow: a weight across an edge is e^-64 / 256 and less, and its square lies below float32's range.  A product that underflows carries an ABSOLUTE
             error of at most TINY = 2^-126 (the smallest normal number: gradual underflow rounds finer, a flush to zero loses no more), whatever its size:
             per tap TINY (1 + v(q)) / sw^2 on the variance and TINY / sw on the colour.  These terms are of the order 1e-35.
             No pixel is excluded.  Each stage is compared from the device's own input to that stage, so no bar compounds.

level32      a float32 numpy model of one level, for the CPU test: np.exp rounded to float32 stands in for skh_libm's exp (inside the 3.2 u the bar grants).  Its
             `mutate` argument breaks one line at a time."""
import numpy as np

from tests import denoiseref as D
from tests import temporalref as T
from tests.denoiseref import modulation, surface_mask

U = 2.0 ** -24
DEMODULATE, REMODULATE, ESTIMATE = 1, 2, 4
COEF = (np.float32(0.2126), np.float32(0.7152), np.float32(0.0722))
G3 = (0.25, 0.5, 0.25)
K_EST, K_VAR = 99.0, 53.0
EXP_ALONE = 2.2 * U
REL_KL = 13.5 * U
TINY = 2.0 ** -126


def lum32(c):
    c = np.asarray(c, np.float32)
    return (COEF[0] * c[..., 0] + COEF[1] * c[..., 1]) + COEF[2] * c[..., 2]


def lum64(c):
    """(lum, sum |coef c|) in float64 with the float32 coefficients"""
    c = np.asarray(c, np.float64)
    k = [float(x) for x in COEF]
    return k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2], k[0] * np.abs(c[..., 0]) + k[1] * np.abs(c[..., 1]) + k[2] * np.abs(c[..., 2])


def vparams(width, height, first_level=0, levels=1, sigma_luminance=4.0, sigma_normal=0.3, sigma_plane=0.05, albedo_floor=0.05, epsilon=1e-2, min_history=4.0, flags=0):
    from strelka_amd import scene as S

    return S.vdenoise_params(width, height, levels=levels, sigma_luminance=sigma_luminance, sigma_normal=sigma_normal, sigma_plane=sigma_plane,
                             first_level=first_level, albedo_floor=albedo_floor, epsilon=epsilon, min_history=min_history, demodulate=bool(flags & DEMODULATE),
                             remodulate=bool(flags & REMODULATE), estimate=bool(flags & ESTIMATE))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_moments
# ---------------------------------------------------------------------------------------------------------------------------------------------
def mask_of(motion):
    """the definition's mask = (motion.w >= 0 && motion.w <= 15) ? (uint)motion.w : 0"""
    mw = np.asarray(motion, np.float32)[..., 3]
    with np.errstate(invalid="ignore"):
        ok = (mw >= np.float32(0.0)) & (mw <= np.float32(15.0))
    return np.where(ok, np.where(ok, mw, 0.0).astype(np.uint32), np.uint32(0)).astype(np.uint32)


def moments32(color, ids, position, albedo, motion, prev_moments, p):
    """the definition in float32.  Planes (h, w, 4) as the device gets them; motion and prev_moments both None: no previous frame -> (h, w, 4) float32"""
    f = np.float32
    C, ids = np.asarray(color, f), np.asarray(ids, np.uint32)
    h, w = C.shape[:2]
    surf = surface_mask(C, ids)
    P0, P1, P2 = (np.asarray(position, f)[..., k] for k in range(3))
    with np.errstate(all="ignore"):
        c = C[..., :3]
        if int(p["flags"]) & DEMODULATE:
            c = c / modulation(albedo, p["albedo_floor"])
        l = lum32(c)
        ll = l * l
        m1, m2, nn = l, ll, np.full((h, w), f(p["initial_length"]), f)
        if prev_moments is not None:
            mask = mask_of(motion)
            M = np.asarray(p["prev_world_to_clip"], f).reshape(16)
            row = lambda r: ((M[4 * r] * P0 + M[4 * r + 1] * P1) + M[4 * r + 2] * P2) + M[4 * r + 3] * f(1.0)
            clx, cly, clw = row(0), row(1), row(3)
            W, H = f(w), f(h)
            fx = ((clx / clw) * f(0.5) + f(0.5)) * W - f(0.5)
            fy = ((cly / clw) * f(0.5) + f(0.5)) * H - f(0.5)
            proj = (clw > f(0.0)) & np.isfinite(fx) & np.isfinite(fy) & (fx >= f(-1.0)) & (fx <= W) & (fy >= f(-1.0)) & (fy <= H)
            yy, xx = np.mgrid[0:h, 0:w]
            gx, gy = np.where(proj, fx, xx.astype(f)), np.where(proj, fy, yy.astype(f))
            flx, fly = np.floor(gx), np.floor(gy)
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            tx, ty = gx - flx, gy - fly
            ux, uy = f(1.0) - tx, f(1.0) - ty
            wk = (ux * uy, tx * uy, ux * ty, tx * ty)
            PM = np.asarray(prev_moments, f)
            sw, s1, s2, sn = (np.zeros((h, w), f) for _ in range(4))
            anyt = np.zeros((h, w), bool)
            for k, (dx, dy) in enumerate(T.TAPS):
                qx, qy = ix + dx, iy + dy
                inb = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                mq = PM[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                used = (proj & (((mask >> np.uint32(k)) & 1) != 0) & inb & (wk[k] > f(0.0)) & np.isfinite(mq[..., 0]) & np.isfinite(mq[..., 1]) & np.isfinite(mq[..., 3])
                        & (mq[..., 3] >= f(1.0)))
                sw = np.where(used, sw + wk[k], sw)
                s1 = np.where(used, s1 + wk[k] * mq[..., 0], s1)
                s2 = np.where(used, s2 + wk[k] * mq[..., 1], s2)
                sn = np.where(used, sn + wk[k] * mq[..., 3], sn)
                anyt |= used
            h1, h2, nh = s1 / sw, s2 / sw, sn / sw
            n1 = nh + f(1.0)
            nb = np.where(n1 < f(p["max_history"]), n1, f(p["max_history"]))
            alpha = f(1.0) / nb
            m1 = np.where(anyt, h1 + (l - h1) * alpha, l)
            m2 = np.where(anyt, h2 + (ll - h2) * alpha, ll)
            nn = np.where(anyt, nb, nn)
        v = m2 - m1 * m1
        v = np.where(v > f(0.0), v, f(0.0))
        out = np.stack([m1, m2, v, nn], -1).astype(f)
    return np.where(surf[..., None], out, f(0.0)).astype(f)


def moments64(color, ids, position, albedo, motion, prev_moments, p):
    """float64 on the float32 planes -> {"moments", "bar": (h, w, 4), "surface", "ambiguous", "used": (h, w) the number of used taps}"""
    f, d64 = np.float32, np.float64
    C, ids = np.asarray(color, f), np.asarray(ids, np.uint32)
    h, w = C.shape[:2]
    surf = surface_mask(C, ids)
    P = np.asarray(position, d64)[..., :3]
    with np.errstate(all="ignore"):
        c32 = C[..., :3]
        if int(p["flags"]) & DEMODULATE:
            c32 = (c32 / modulation(albedo, p["albedo_floor"])).astype(f)  # (one correctly rounded float32 division: the device's bits)
        c = np.where(surf[..., None], c32, 0.0).astype(d64)
        l, L = lum64(c)
        el = 5 * U * L
        ll = l * l
        ell = 2 * np.abs(l) * el + el * el + U * ll
        m1, e1, m2, e2 = l, el, ll, ell
        nn, e_nn = np.full((h, w), float(f(p["initial_length"]))), np.zeros((h, w))
        ambiguous, count = np.zeros((h, w), bool), np.zeros((h, w), int)
        if prev_moments is not None:
            mask = mask_of(motion)
            M = np.asarray(p["prev_world_to_clip"], f).astype(d64).reshape(4, 4)
            row = lambda r: M[r, 0] * P[..., 0] + M[r, 1] * P[..., 1] + M[r, 2] * P[..., 2] + M[r, 3]
            mag = lambda r: 4 * U * (np.abs(M[r, 0] * P[..., 0]) + np.abs(M[r, 1] * P[..., 1]) + np.abs(M[r, 2] * P[..., 2]) + np.abs(M[r, 3]))
            clw, ew = row(3), mag(3)
            amb_w = np.abs(clw) < ew
            W, H = float(w), float(h)

            def axis(r, S):
                cl, ec = row(r), mag(r)
                q = cl / clw
                g = q * 0.5 + 0.5
                fv = g * S - 0.5
                return fv, S * ((ec + np.abs(q) * ew) / (2 * np.abs(clw)) + U * np.abs(q) / 2 + U * np.abs(g)) + U * np.abs(g) * S + 2 * U * np.abs(fv)

            (fx, efx), (fy, efy) = axis(0, W), axis(1, H)
            infront = clw > 0
            inrange = np.isfinite(fx) & np.isfinite(fy) & (fx >= -1) & (fx <= W) & (fy >= -1) & (fy <= H)
            amb_r = infront & ~amb_w & np.isfinite(fx) & np.isfinite(fy) & ((np.abs(fx + 1) < efx) | (np.abs(W - fx) < efx) | (np.abs(fy + 1) < efy) | (np.abs(H - fy) < efy))
            proj = infront & inrange
            yy, xx = np.mgrid[0:h, 0:w]
            gx, gy = np.where(proj, fx, xx.astype(d64)), np.where(proj, fy, yy.astype(d64))
            flx, fly = np.floor(gx), np.floor(gy)
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            tx, ty = gx - flx, gy - fly
            amb_f = proj & ((np.minimum(tx, 1 - tx) < efx) | (np.minimum(ty, 1 - ty) < efy))
            ux, uy = 1 - tx, 1 - ty
            etx, ety = efx + U, efy + U
            wk = (ux * uy, tx * uy, ux * ty, tx * ty)
            ek = (etx * uy + ety * ux, etx * uy + ety * tx, etx * ty + ety * ux, etx * ty + ety * tx)
            PM = np.asarray(prev_moments, f)
            sw = np.zeros((h, w))
            s = [np.zeros((h, w)) for _ in range(3)]
            sabs = [np.zeros((h, w)) for _ in range(3)]
            taps = []
            anyt = np.zeros((h, w), bool)
            for k, (dx, dy) in enumerate(T.TAPS):
                qx, qy = ix + dx, iy + dy
                inb = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                mq32 = PM[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                used = (proj & (((mask >> np.uint32(k)) & 1) != 0) & inb & (wk[k] > 0) & np.isfinite(mq32[..., 0]) & np.isfinite(mq32[..., 1])
                        & np.isfinite(mq32[..., 3]) & (mq32[..., 3] >= f(1.0)))
                mq = np.where(used[..., None], mq32, 0.0).astype(d64)[..., [0, 1, 3]]
                wq, eq = np.where(used, wk[k], 0.0), np.where(used, ek[k] + U * wk[k], 0.0)
                sw += wq
                for j in range(3):
                    s[j] += wq * mq[..., j]
                    sabs[j] += wq * np.abs(mq[..., j])
                anyt |= used
                count += used
                taps.append((eq, mq))
            den = np.where(anyt, sw, 1.0)
            hm = [s[j] / den for j in range(3)]
            eh = []
            for j in range(3):
                wpart = np.zeros((h, w))
                for eq, mq in taps:
                    wpart += eq * np.abs(mq[..., j] - hm[j])
                eh.append(9 * U * sabs[j] / den + 2 * wpart / den)
            maxh = float(f(p["max_history"]))
            n1 = hm[2] + 1.0
            nb = np.minimum(n1, maxh)
            e_nb = eh[2] + U * n1
            alpha = 1.0 / nb

            def blend(m, em, x, ex):
                b = m + (x - m) * alpha
                return b, em + alpha * ex + alpha * np.abs(x - m) * (e_nb / nb + 3 * U) + 2 * U * (np.abs(m) + alpha * np.abs(x - m))

            b1, eb1 = blend(hm[0], eh[0], l, el)
            b2, eb2 = blend(hm[1], eh[1], ll, ell)
            m1, e1 = np.where(anyt, b1, l), np.where(anyt, eb1, el)
            m2, e2 = np.where(anyt, b2, ll), np.where(anyt, eb2, ell)
            nn, e_nn = np.where(anyt, nb, nn), np.where(anyt, e_nb, 0.0)
            ambiguous = surf & (mask != 0) & (amb_w | amb_r | (~amb_w & ~amb_r & amb_f))
        v = m2 - m1 * m1
        ev = e2 + 2 * np.abs(m1) * e1 + e1 * e1 + 2 * U * (np.abs(m2) + m1 * m1)
        v = np.maximum(v, 0.0)
    s4 = surf[..., None]
    return {"moments": np.where(s4, np.stack([m1, m2, v, nn], -1), 0.0), "bar": np.where(s4, np.stack([e1, e2, ev, e_nn], -1), 0.0), "surface": surf,
            "ambiguous": ambiguous, "used": np.where(surf, count, 0)}


def check_moments(got, ref):
    """worst |got - ref| / bar over the unambiguous surface pixels (0 where both are 0); pixels that are no surface pixels must be {0, 0, 0, 0}"""
    got = np.asarray(got, np.float32)
    surf, use = ref["surface"], ref["surface"] & ~ref["ambiguous"]
    assert not got[~surf].view(np.uint32).any(), "a pixel that is no surface pixel has moments"
    g = got.astype(np.float64)[use]
    assert np.isfinite(g).all(), "a non-finite moment on a surface pixel"
    assert (g[:, 2] >= 0).all(), "a negative variance"
    err, bar = np.abs(g - ref["moments"][use]), ref["bar"][use]
    ratio = np.where(err == 0.0, 0.0, err / np.where(bar > 0.0, bar, np.finfo(np.float64).tiny))
    return float(ratio.max()) if ratio.size else 0.0


def synthetic_moments(width=67, height=45, seed=11):
    """temporalref.synthetic (its camera pair) plus "motion" -- what skh_temporal writes for it (reproject32's) -- and "prev_moments": random positive mu1,
    mu2 >= mu1^2, nm in 1 .. 32, {0, 0, 0, 0} where the previous frame has no surface, and a sprinkle of NaN / nm 0 records"""
    s = T.synthetic(width, height)
    rs = np.random.RandomState(seed)
    h, w = height, width
    mu1 = rs.uniform(0.2, 1.5, (h, w))
    PM = np.zeros((h, w, 4), np.float32)
    PM[..., 0] = mu1
    PM[..., 1] = mu1 * mu1 + rs.uniform(0.0, 0.3, (h, w))
    PM[..., 2] = PM[..., 1] - PM[..., 0] * PM[..., 0]
    PM[..., 3] = rs.randint(1, 33, (h, w))
    r = rs.uniform(size=(h, w))
    PM[r < 0.02, 3] = 0.0
    PM[(r >= 0.02) & (r < 0.03), 0] = np.nan
    PM[(r >= 0.03) & (r < 0.04), 1] = np.inf
    PM[(r >= 0.04) & (r < 0.05), 3] = np.nan
    pk = s["prev"]["ids"][..., 3]
    PM[~((pk == 1) | (pk == 2))] = 0.0
    s["prev_moments"] = PM
    s["motion"] = T.reproject32(s["color"], s["ids"], s["normal"], s["position"], s["albedo"], s["prev"], s["params"])["motion"]
    return s


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_denoise_variance
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pack(color, ids, albedo, moments, p):
    """the first level's input as the device packs it: (c (h, w, 3) float32 -- demodulated with the flag --, v0 (h, w) float32 WITHOUT the estimate, valid)"""
    f = np.float32
    color = np.asarray(color, f)
    valid = surface_mask(color, ids)
    c32 = color[..., :3].copy()
    with np.errstate(all="ignore"):
        if int(p["flags"]) & DEMODULATE:
            c32 = np.where(valid[..., None], c32 / modulation(albedo, p["albedo_floor"]), c32).astype(f)
        z = np.asarray(moments, f)[..., 2]
        v0 = np.where(np.isfinite(z) & (z > f(0.0)), z, f(0.0)).astype(f)
    return np.where(valid[..., None], c32, f(0.0)), np.where(valid, v0, f(0.0)), valid


def _guide_terms(N, P, Nq, Pq, kn, kp):
    """tn, tp and the bar of their float32 values without the additions that join them (denoiseref.level's count)"""
    n = Nq - N
    tn = (n * n).sum(-1) * kn
    g = Pq - P
    d = (N * g).sum(-1)
    D1 = np.abs(N * g).sum(-1)
    tp = d * d * kp
    return tn, tp, 8 * U * tn + kp * (8 * U * np.abs(d) * D1 + 16 * U * U * D1 * D1) + 4 * U * tp


def _shift(yy, xx, dy, dx, h, w):
    qy, qx = yy + dy, xx + dx
    inb = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
    return np.where(inb, qy, yy), np.where(inb, qx, xx), inb


def estimate64(v0, valid, N, P, moments, p):
    """the input variance with SKH_VDENOISE_ESTIMATE.  v0, valid: pack()'s; moments the (h, w, 4) float32 plane -> (v (h, w) float64, bar (h, w))"""
    f = np.float32
    N, P = np.asarray(N, np.float64)[..., :3], np.asarray(P, np.float64)[..., :3]
    M = np.asarray(moments, f)
    h, w = valid.shape
    kn, kp = D.inv_sq(p["sigma_normal"]), D.inv_sq(p["sigma_plane"])
    minh = float(f(p["min_history"]))
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        nm = M[..., 3]
        takes = valid & ~(nm >= f(minh))
        s0 = np.zeros((h, w))
        s, sabs = [np.zeros((h, w)), np.zeros((h, w))], [np.zeros((h, w)), np.zeros((h, w))]
        taps = []
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qy, qx, inb = _shift(yy, xx, dy, dx, h, w)
                mq32 = M[qy, qx]
                take = inb & valid[qy, qx] & valid & np.isfinite(mq32[..., 0]) & np.isfinite(mq32[..., 1])
                mq = np.where(take[..., None], mq32, 0.0).astype(np.float64)
                tn, tp, da = _guide_terms(N, P, N[qy, qx], P[qy, qx], kn, kp)
                a = tn + tp
                da = da + U * a
                da = np.where(a - da >= 64.0, 0.0, da)
                da = np.where(np.isfinite(da), da, 0.0)
                wq = np.where(take, np.exp(-np.where(a <= 64.0, a, 64.0)), 0.0)
                dw = np.where(take, np.expm1(da) + EXP_ALONE, 0.0)
                s0 += wq
                for j in range(2):
                    s[j] += wq * mq[..., j]
                    sabs[j] += wq * np.abs(mq[..., j])
                taps.append((wq * dw, mq))
        anyt = s0 > 0
        den = np.where(anyt, s0, 1.0)
        e = [s[j] / den for j in range(2)]
        b = []
        for j in range(2):
            wpart = np.zeros((h, w))
            for wdw, mq in taps:
                wpart += wdw * np.abs(mq[..., j] - e[j])
            b.append(K_EST * U * sabs[j] / den + 2.0 * wpart / den)
        v = e[1] - e[0] * e[0]
        ev = b[1] + 2 * np.abs(e[0]) * b[0] + b[0] * b[0] + 2 * U * (np.abs(e[1]) + e[0] * e[0])
        v = np.maximum(v, 0.0)
        k = minh / np.where(nm >= f(1.0), nm, f(1.0)).astype(np.float64)
        vk, evk = v * k, ev * k + 3 * U * v * k
        out = np.where(takes, np.where(anyt, vk, 0.0), np.asarray(v0, np.float64))
        bar = np.where(takes & anyt, evk, 0.0)
    return np.where(valid, out, 0.0), np.where(valid, bar, 0.0)


def level64(c, v, valid, N, P, lvl, p):
    """one level from the level's input colour c (h, w, 3) and variance v (h, w) (the device's float32 values) -> (out (h, w, 3), bar, vout (h, w), vbar_)"""
    c, v, N, P = (np.asarray(a, np.float64) for a in (c, v, np.asarray(N)[..., :3], np.asarray(P)[..., :3]))
    h, w = valid.shape
    s = 1 << lvl
    sl = float(np.float32(p["sigma_luminance"]))
    eps = float(np.float32(p["epsilon"]))
    kn, kp = D.inv_sq(p["sigma_normal"]), D.inv_sq(p["sigma_plane"])
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        bv, bk = np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx, inb = _shift(yy, xx, dy, dx, h, w)
                take = inb & valid[qy, qx] & valid
                k = G3[dx + 1] * G3[dy + 1]
                bv += np.where(take, k * v[qy, qx], 0.0)
                bk += np.where(take, k, 0.0)
        vb = bv / np.where(valid, bk, 1.0)
        lum_off = np.isinf(sl)
        kl = np.zeros((h, w)) if lum_off else 1.0 / (sl * np.sqrt(vb) + eps)
        lp, Lp = lum64(c)
        sw, sv, under = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        sc, sabs = np.zeros((h, w, 3)), np.zeros((h, w, 3))
        taps = []
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx, inb = _shift(yy, xx, dy * s, dx * s, h, w)
                take = inb & valid[qy, qx] & valid
                cq, vq = c[qy, qx], v[qy, qx]
                tn, tp, dg = _guide_terms(N, P, N[qy, qx], P[qy, qx], kn, kp)
                if lum_off:
                    tl, dtl = np.zeros((h, w)), np.zeros((h, w))
                else:
                    tl = np.abs(lp[qy, qx] - lp) * kl
                    dtl = kl * 5 * U * (Lp[qy, qx] + Lp) + (REL_KL + 2 * U) * tl
                a = tl + tn + tp
                da = dtl + dg + 2 * U * a
                da = np.where(a - da >= 64.0, 0.0, da)
                da = np.where(np.isfinite(da), da, 0.0)
                wq = D.H5[dx + 2] * D.H5[dy + 2] * np.exp(-np.where(a <= 64.0, a, 64.0))
                dw = np.where(take, np.expm1(da) + D.EXP_AND_PRODUCT, 0.0)
                wq = np.where(take, wq, 0.0)
                cq, vq = np.where(take[..., None], cq, 0.0), np.where(take, vq, 0.0)
                sw += wq
                sc += wq[..., None] * cq
                sabs += wq[..., None] * np.abs(cq)
                sv += wq * wq * vq
                under += np.where(take, TINY * (1.0 + vq), 0.0)
                taps.append((wq, dw, cq, vq))
        den = np.where(valid, sw, 1.0)
        out = sc / den[..., None]
        vout = sv / (den * den)
        wpart, vpart = np.zeros((h, w, 3)), np.zeros((h, w))
        for wq, dw, cq, vq in taps:
            wpart += (wq * dw)[..., None] * np.abs(cq - out)
            vpart += wq * dw * np.abs(wq * vq - vout * den)
        bar = D.K_SUMS * U * sabs / den[..., None] + 2.0 * wpart / den[..., None] + (25 * TINY / den)[..., None]
        vbar_ = K_VAR * U * vout + 4.0 * vpart / (den * den) + under / (den * den)
    m3 = valid[..., None]
    return np.where(m3, out, 0.0), np.where(m3, bar, 0.0), np.where(valid, vout, 0.0), np.where(valid, vbar_, 0.0)


def exp32(x):
    """np.exp rounded to float32: the stand-in for skh_libm's exp"""
    return np.exp(np.asarray(x, np.float64)).astype(np.float32)


def level32(c, v, valid, N, P, lvl, p, mutate=None):
    """a float32 model of one level, operation by operation -> (out (h, w, 3) float32, vout (h, w) float32).  mutate: None, "w_for_ww" (w in place of w w in the
    variance sum), "v_for_vbar" (v(p) in place of vbar), "no_root" (sqrt dropped)"""
    f = np.float32
    c, v, N, P = np.asarray(c, f), np.asarray(v, f), np.asarray(N, f)[..., :3], np.asarray(P, f)[..., :3]
    h, w = valid.shape
    s = 1 << lvl
    sl, eps = f(p["sigma_luminance"]), f(p["epsilon"])
    kn = f(1.0) / (f(p["sigma_normal"]) * f(p["sigma_normal"]))
    kp = f(1.0) / (f(p["sigma_plane"]) * f(p["sigma_plane"]))
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        bv, bk = np.zeros((h, w), f), np.zeros((h, w), f)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx, inb = _shift(yy, xx, dy, dx, h, w)
                take = inb & valid[qy, qx]
                k = f(G3[dx + 1]) * f(G3[dy + 1])
                bv = np.where(take, bv + k * v[qy, qx], bv)
                bk = np.where(take, bk + k, bk)
        vb = bv / bk
        if mutate == "v_for_vbar":
            vb = v
        root = vb if mutate == "no_root" else np.sqrt(vb)
        lum_off = np.isinf(sl)
        kl = None if lum_off else f(1.0) / (sl * root + eps)
        lp = lum32(c)
        sw, sv = np.zeros((h, w), f), np.zeros((h, w), f)
        sc = np.zeros((h, w, 3), f)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx, inb = _shift(yy, xx, dy * s, dx * s, h, w)
                take = inb & valid[qy, qx]
                cq, vq, Nq, Pq = c[qy, qx], v[qy, qx], N[qy, qx], P[qy, qx]
                n = Nq - N
                tn = ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]) * kn
                g = Pq - P
                d = (N[..., 0] * g[..., 0] + N[..., 1] * g[..., 1]) + N[..., 2] * g[..., 2]
                tp = (d * d) * kp
                tl = np.zeros((h, w), f) if lum_off else np.abs(lum32(cq) - lp) * kl
                a = (tl + tn) + tp
                a = np.where(a <= f(64.0), a, f(64.0))
                wq = (f(D.H5[dx + 2]) * f(D.H5[dy + 2])) * exp32(-a)
                sw = np.where(take, sw + wq, sw)
                sc = np.where(take[..., None], sc + wq[..., None] * cq, sc)
                ww = wq if mutate == "w_for_ww" else wq * wq
                sv = np.where(take, sv + ww * vq, sv)
        out = sc / sw[..., None]
        vout = sv / (sw * sw)
    return np.where(valid[..., None], out, f(0.0)).astype(f), np.where(valid, vout, f(0.0)).astype(f)


def worst(got, ref, bar, where):
    """max |got - ref| / bar over `where` (0 where the error is 0)"""
    with np.errstate(invalid="ignore"):
        g = np.asarray(got, np.float64)[where]
    assert np.isfinite(g).all(), "a non-finite value on a surface pixel"
    err, b = np.abs(g - ref[where]), bar[where]
    ratio = np.where(err == 0.0, 0.0, err / np.where(b > 0.0, b, np.finfo(np.float64).tiny))
    return float(ratio.max()) if ratio.size else 0.0


def synthetic(width=67, height=45, seed=7, special=True):
    """denoiseref.synthetic plus a "moments" plane: mu1 near the demodulated luminance, mu2 >= mu1^2, a variance that changes across the image by a factor of
    100 (with zeros, a negative, a NaN and an Inf among them), nm in 0 .. 32 with a quarter of the pixels below 4 and a sprinkle of NaN moments"""
    s = D.synthetic(width, height, special=special)
    rs = np.random.RandomState(seed)
    h, w = height, width
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    mu1 = 0.6 + 0.3 * np.sin(x * 0.11) * np.cos(y * 0.07) + rs.uniform(-0.05, 0.05, (h, w))
    var = 0.002 * 10.0 ** (2.0 * rs.uniform(size=(h, w)) * (0.5 + 0.5 * np.sin(x * 0.3)))
    M = np.zeros((h, w, 4), np.float32)
    M[..., 0], M[..., 1], M[..., 2] = mu1, mu1 * mu1 + var, var
    M[..., 3] = np.where(rs.uniform(size=(h, w)) < 0.25, rs.randint(0, 4, (h, w)), rs.randint(4, 33, (h, w)))
    r = rs.uniform(size=(h, w))
    M[r < 0.02, 2] = 0.0
    if special and h > 8 and w > 8:
        M[3, 3, 2], M[4, 7, 2], M[6, 2, 2] = -1.0, np.nan, np.inf
        M[8, 5, 0], M[2, 8, 1], M[7, 7, 3] = np.nan, np.inf, np.nan
    s["moments"] = M
    return s
