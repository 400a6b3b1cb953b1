"""Temporal accumulation's definition (include/strelka_hip.h, "Temporal accumulation") in numpy, twice.

reproject32   the definition restated operation by operation in float32.  It has no transcendental: + - x /, floor, compare and select, each of which numpy's
              float32 rounds as IEEE 754 says -- as the device does with contraction off and its correctly rounded division.  The device must give these bits.

reproject64   the same definition in float64 on the same float32 planes, with a per-pixel error bar for the float32 evaluation that is a written-out count of
              roundings, as tests/denoiseref.py does it.  u = 2^-24 is float32's unit roundoff; "4 u D" for a three-term dot product means: three products and
              two additions whose partial sums are at most D = the sum of the terms' magnitudes, one u spare.

  decisions   A float32 evaluation may decide differently from float64 where a quantity lies within its rounding error of the threshold.  Per pixel the margin of
              every decision is compared with that decision's bar; a pixel with a margin below its bar is AMBIGUOUS and is compared with neither branch.
                clip.w > 0        margin |clip.w|, bar ew = 4 u (|m12 P.x| + |m13 P.y| + |m14 P.z| + |m15|)
                the range test    margin min(fx + 1, W - fx) (and in y), bar efx:
                                  r = clip.x / clip.w carries (ex + |r| ew) / |clip.w| from its operands (ex as ew, of row 0) and u |r| of the quotient; the
                                  product with 0.5 is exact; + 0.5 rounds (u |r/2 + 1/2|); x W rounds (u |..| W); - 0.5 rounds (u |fx|); one u |fx| spare:
                                  efx = W ((ex + |r| ew) / (2 |clip.w|) + u |r| / 2 + u |r/2 + 1/2|) + u |r/2 + 1/2| W + 2 u |fx|
                the two floors    margin min(tx, 1 - tx) (and in y), bar efx: within it the tap set moves by a pixel.  This is also the margin of "weight > 0"
                                  (a weight is a product of tx, 1 - tx, ty, 1 - ty and is 0 only where one of them is) and of "in the image" (a function of the floor)
                the normal test   per tap whose exact tests pass, margin |dot(N', N) - normal_min|, bar 4 u sum |N'_k N_k|
                the plane test    likewise, margin ||d| - plane_tolerance|, bar 4 u sum |N_k g_k|, g_k = P'_k - P_k: per k the difference (u) and the product
                                  (u), and two additions -- denoiseref's count for the same d
              The tests on IDS, on the history's finiteness and on n >= 1 read input words: they have no rounding and no margin.

  the value   on an unambiguous pixel both evaluations take the same taps.
                weights   tx carries efx (fx's error; the subtraction of the floor is exact), 1 - tx one more u: et = efx + u.  w = a b: ew_k = et_x b + et_y a + u w
                h         sum w hist / sum w: with exact weights 9 u S, S = sum w |hist| / sw (the term's product 1, up to 3 additions each for numerator and
                          denominator 6, the quotient 1, one spare); the weights' errors move it by sum ew_k |hist_k - h| / sw to first order, doubled for the rest
                n'        nh as h; + 1 rounds (u (nh + 1)); min is 1-Lipschitz
                ill       h + (c - h) alpha, alpha = 1 / n' (relative error en / n' + u): eh + alpha |c - h| (en / n' + 3 u) + 2 u |ill|
                          (the difference, the product and alpha's quotient 3 u; the sum u, one spare); c is float32's correctly rounded quotient on both sides
                out       ill m: bar m + u |out|
                motion    fx - px: efx + u |fx - px|;  sw: sum ew_k + 3 u sw;  mask: exact
              A pixel without history has ill = c exactly; its out = c m carries u |out|."""
import numpy as np

from tests.denoiseref import modulation, surface_mask

U = 2.0 ** -24
DEMODULATE = 1
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))


def params(width, height, matrix=None, normal_min=0.9, plane_tolerance=0.02, max_history=32.0, initial_length=1.0, albedo_floor=0.05, flags=DEMODULATE):
    from strelka_amd import scene as S

    p = S.temporal_params(width, height, None, normal_min=normal_min, plane_tolerance=plane_tolerance, max_history=max_history, initial_length=initial_length,
                          albedo_floor=albedo_floor, demodulate=bool(flags & DEMODULATE))
    if matrix is not None:
        p["prev_world_to_clip"] = np.asarray(matrix, np.float32).reshape(16)
    return p


def _planes(a, dtype, n):
    return [np.asarray(a, dtype)[..., k] for k in range(n)]


def _compose(C, surf, rgb, hist_rgb, nn, motion):
    """the three float32 images: the values on surface pixels; C's bits, {0,0,0,0} and {0,0,0,0} elsewhere; C's alpha word everywhere"""
    out = np.array(C, np.float32)
    out[..., :3] = np.where(surf[..., None], rgb, out[..., :3])
    history = np.where(surf[..., None], np.concatenate([hist_rgb, nn[..., None]], -1), 0.0).astype(np.float32)
    return {"image": out, "history": history, "motion": np.where(surf[..., None], motion, 0.0).astype(np.float32)}


def reproject32(color, ids, normal, position, albedo, prev, p):
    """the definition in float32.  Planes (h, w, 4) as the device gets them; `prev` None or {"history", "ids", "normal", "position"}; `p` an S.TEMPORAL_PARAMS record
    -> {"image", "history", "motion"}, (h, w, 4) float32"""
    f = np.float32
    C, ids = np.asarray(color, f), np.asarray(ids, np.uint32)
    h, w = C.shape[:2]
    surf = surface_mask(C, ids)
    demod = bool(int(p["flags"]) & DEMODULATE)
    N0, N1, N2 = _planes(normal, f, 3)
    P0, P1, P2 = _planes(position, f, 3)
    with np.errstate(all="ignore"):
        c = C[..., :3]
        if demod:
            m = modulation(albedo, p["albedo_floor"])
            c = c / m
        ill, nn, motion = c, np.full((h, w), f(p["initial_length"]), f), np.zeros((h, w, 4), f)
        if prev is not None:
            M = np.asarray(p["prev_world_to_clip"], f).reshape(16)
            row = lambda r: ((M[4 * r] * P0 + M[4 * r + 1] * P1) + M[4 * r + 2] * P2) + M[4 * r + 3] * f(1.0)
            clx, cly, clw = row(0), row(1), row(3)
            W, H = f(w), f(h)
            fx = ((clx / clw) * f(0.5) + f(0.5)) * W - f(0.5)
            fy = ((cly / clw) * f(0.5) + f(0.5)) * H - f(0.5)
            proj = (clw > f(0.0)) & np.isfinite(fx) & np.isfinite(fy) & (fx >= f(-1.0)) & (fx <= W) & (fy >= f(-1.0)) & (fy <= H)
            yy, xx = np.mgrid[0:h, 0:w]
            px, py = xx.astype(f), yy.astype(f)
            gx, gy = np.where(proj, fx, px), np.where(proj, fy, py)
            flx, fly = np.floor(gx), np.floor(gy)
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            tx, ty = gx - flx, gy - fly
            ux, uy = f(1.0) - tx, f(1.0) - ty
            wk = (ux * uy, tx * uy, ux * ty, tx * ty)
            PH, PI = np.asarray(prev["history"], f), np.asarray(prev["ids"], np.uint32)
            PN, PP = np.asarray(prev["normal"], f), np.asarray(prev["position"], f)
            sw, sn, s3 = np.zeros((h, w), f), np.zeros((h, w), f), np.zeros((h, w, 3), f)
            mask = np.zeros((h, w), np.uint32)
            for k, (dx, dy) in enumerate(TAPS):
                qx, qy = ix + dx, iy + dy
                inb = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ax, ay = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                hq, iq, nq, pq = PH[ay, ax], PI[ay, ax], PN[ay, ax], PP[ay, ax]
                dn = (nq[..., 0] * N0 + nq[..., 1] * N1) + nq[..., 2] * N2
                e0, e1, e2 = pq[..., 0] - P0, pq[..., 1] - P1, pq[..., 2] - P2
                d = (N0 * e0 + N1 * e1) + N2 * e2
                acc = (proj & inb & (wk[k] > f(0.0)) & (iq[..., 3] == ids[..., 3]) & (iq[..., 0] == ids[..., 0]) & np.isfinite(hq).all(-1) & (hq[..., 3] >= f(1.0))
                       & (dn >= f(p["normal_min"])) & (np.abs(d) <= f(p["plane_tolerance"])))
                sw = np.where(acc, sw + wk[k], sw)
                s3 = np.where(acc[..., None], s3 + wk[k][..., None] * hq[..., :3], s3)
                sn = np.where(acc, sn + wk[k] * hq[..., 3], sn)
                mask |= acc.astype(np.uint32) << np.uint32(k)
            hh, nh = s3 / sw[..., None], sn / sw
            n1 = nh + f(1.0)
            nb = np.where(n1 < f(p["max_history"]), n1, f(p["max_history"]))
            alpha = f(1.0) / nb
            anyt = mask != 0
            ill = np.where(anyt[..., None], hh + (c - hh) * alpha[..., None], c)
            nn = np.where(anyt, nb, nn)
            motion = np.where(proj[..., None], np.stack([fx - px, fy - py, sw, mask.astype(f)], -1), f(0.0))
        rgb = ill * m if demod else ill
    return _compose(C, surf, rgb, ill, nn, motion)


def reproject64(color, ids, normal, position, albedo, prev, p):
    """the definition in float64 on the float32 planes -> {"image", "history", "motion": (h, w, 4) float64, "bar_image", "bar_history", "bar_motion": (h, w, 4),
    "surface", "ambiguous", "projects": (h, w) bool, "accepted": (h, w) int, the number of accepted taps}"""
    f, d64 = np.float32, np.float64
    C, ids = np.asarray(color, f), np.asarray(ids, np.uint32)
    h, w = C.shape[:2]
    surf = surface_mask(C, ids)
    demod = bool(int(p["flags"]) & DEMODULATE)
    N = np.asarray(normal, d64)[..., :3]
    P = np.asarray(position, d64)[..., :3]
    with np.errstate(all="ignore"):
        c32 = C[..., :3]
        m = np.ones((h, w, 3))
        if demod:
            m32 = modulation(albedo, p["albedo_floor"])
            c32 = (c32 / m32).astype(f)  # (one correctly rounded float32 division: the device's bits)
            m = m32.astype(d64)
        c = np.where(surf[..., None], c32, 0.0).astype(d64)
        ill, e_ill = c, np.zeros((h, w, 3))
        nn, e_nn = np.full((h, w), float(f(p["initial_length"]))), np.zeros((h, w))
        motion, e_motion = np.zeros((h, w, 4)), np.zeros((h, w, 4))
        ambiguous, proj, count = np.zeros((h, w), bool), np.zeros((h, w), bool), np.zeros((h, w), int)
        if prev is not None:
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
                efv = S * ((ec + np.abs(q) * ew) / (2 * np.abs(clw)) + U * np.abs(q) / 2 + U * np.abs(g)) + U * np.abs(g) * S + 2 * U * np.abs(fv)
                return fv, efv

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
            PH, PI = np.asarray(prev["history"], f), np.asarray(prev["ids"], np.uint32)
            PN, PP = np.asarray(prev["normal"], d64)[..., :3], np.asarray(prev["position"], d64)[..., :3]
            sw, sn, s3 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
            sabs3, sabsn, sek = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
            amb_t = np.zeros((h, w), bool)
            mask = np.zeros((h, w), np.uint32)
            taps = []
            for k, (dx, dy) in enumerate(TAPS):
                qx, qy = ix + dx, iy + dy
                inb = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                ax, ay = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                hq32, iq, nq, pq = PH[ay, ax], PI[ay, ax], PN[ay, ax], PP[ay, ax]
                exact = proj & inb & (wk[k] > 0) & (iq[..., 3] == ids[..., 3]) & (iq[..., 0] == ids[..., 0]) & np.isfinite(hq32).all(-1) & (hq32[..., 3] >= f(1.0))
                hq = np.where(exact[..., None], hq32, 0.0).astype(d64)
                dn = (nq * N).sum(-1)
                e_dn = 4 * U * np.abs(nq * N).sum(-1)
                g = pq - P
                d = (N * g).sum(-1)
                e_d = 4 * U * np.abs(N * g).sum(-1)
                nmin, tol = float(f(p["normal_min"])), float(f(p["plane_tolerance"]))
                ok_n, ok_p = dn >= nmin, np.abs(d) <= tol
                near_n = np.abs(dn - nmin) < e_dn
                near_p = (np.abs(np.abs(d) - tol) < e_d) if np.isfinite(tol) else np.zeros((h, w), bool)
                # (a tap that one test rejects beyond its bar is rejected whatever the other says)
                amb_t |= exact & ((near_n & (ok_p | near_p)) | (near_p & (ok_n | near_n)))
                acc = exact & ok_n & ok_p
                wq, eq = np.where(acc, wk[k], 0.0), np.where(acc, ek[k] + U * wk[k], 0.0)
                hq = np.where(acc[..., None], hq, 0.0)
                sw += wq
                s3 += wq[..., None] * hq[..., :3]
                sn += wq * hq[..., 3]
                sabs3 += wq[..., None] * np.abs(hq[..., :3])
                sabsn += wq * np.abs(hq[..., 3])
                sek += eq
                mask |= acc.astype(np.uint32) << np.uint32(k)
                taps.append((eq, hq))
            anyt = mask != 0
            den = np.where(anyt, sw, 1.0)
            hh, nh = s3 / den[..., None], sn / den
            wpart3, wpartn = np.zeros((h, w, 3)), np.zeros((h, w))
            for eq, hq in taps:
                wpart3 += eq[..., None] * np.abs(hq[..., :3] - hh)
                wpartn += eq * np.abs(hq[..., 3] - nh)
            e_h = 9 * U * sabs3 / den[..., None] + 2 * wpart3 / den[..., None]
            e_nh = 9 * U * sabsn / den + 2 * wpartn / den
            maxh = float(f(p["max_history"]))
            n1 = nh + 1.0
            nb = np.minimum(n1, maxh)
            e_nb = e_nh + U * n1
            alpha = 1.0 / nb
            blend = hh + (c - hh) * alpha[..., None]
            e_blend = e_h + (alpha * (e_nb / nb + 3 * U))[..., None] * np.abs(c - hh) + 2 * U * np.abs(blend)
            ill, e_ill = np.where(anyt[..., None], blend, c), np.where(anyt[..., None], e_blend, 0.0)
            nn, e_nn = np.where(anyt, nb, nn), np.where(anyt, e_nb, 0.0)
            pj = proj[..., None]
            motion = np.where(pj, np.stack([fx - xx, fy - yy, sw, mask.astype(d64)], -1), 0.0)
            e_motion = np.where(pj, np.stack([efx + U * np.abs(fx - xx), efy + U * np.abs(fy - yy), sek + 3 * U * sw, np.zeros((h, w))], -1), 0.0)
            # the first decision that is in doubt settles it; later ones are looked at only where the earlier ones are clear
            ambiguous = surf & (amb_w | amb_r | (~amb_w & ~amb_r & (amb_f | amb_t)))
            count = np.array([(mask >> k) & 1 for k in range(4)]).sum(0).astype(int)
        rgb = ill * m
        e_rgb = e_ill * m + (U * np.abs(rgb) if demod else 0.0)
    s3_ = surf[..., None]
    z1 = np.zeros((h, w, 1))
    image = np.concatenate([np.where(s3_, rgb, 0.0), z1], -1)
    history = np.where(s3_, np.concatenate([ill, nn[..., None]], -1), 0.0)
    return {"image": image, "history": history, "motion": np.where(s3_, motion, 0.0),
            "bar_image": np.concatenate([np.where(s3_, e_rgb, 0.0), z1], -1),
            "bar_history": np.where(s3_, np.concatenate([e_ill, e_nn[..., None]], -1), 0.0), "bar_motion": np.where(s3_, e_motion, 0.0),
            "surface": surf, "ambiguous": ambiguous, "projects": proj & surf, "accepted": np.where(surf, count, 0)}


def check(got, color, ref):
    """`got`: {"image", "history", "motion"} float32 for the input `color`.  Asserts the bit-exact parts -- the alpha word everywhere, every word of a pixel that is
    no surface pixel, the mask word -- and returns the worst |got - ref| / bar over the unambiguous surface pixels, all three images (0 where both are 0)."""
    color = np.asarray(color, np.float32)
    surf, use = ref["surface"], ref["surface"] & ~ref["ambiguous"]
    img = np.asarray(got["image"], np.float32)
    assert np.array_equal(img[..., 3].view(np.uint32), color[..., 3].view(np.uint32)), "an alpha word changed"
    assert np.array_equal(img[~surf].view(np.uint32), color[~surf].view(np.uint32)), "a pixel that is no surface pixel changed"
    assert not np.asarray(got["history"])[~surf].any() and not np.asarray(got["motion"])[~surf].any(), "a pixel that is no surface pixel has history or motion"
    assert np.array_equal(np.asarray(got["motion"])[use][:, 3], ref["motion"][use][:, 3]), "the tap masks differ on an unambiguous pixel"
    worst = 0.0
    for name, channels in (("image", 3), ("history", 4), ("motion", 3)):
        with np.errstate(invalid="ignore"):
            g = np.asarray(got[name], np.float64)[use][:, :channels]
        assert np.isfinite(g).all(), f"a non-finite value in {name} on a surface pixel"
        err, bar = np.abs(g - ref[name][use][:, :channels]), ref["bar_" + name][use][:, :channels]
        ratio = np.where(err == 0.0, 0.0, err / np.where(bar > 0.0, bar, np.finfo(np.float64).tiny))
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the synthetic input
# ---------------------------------------------------------------------------------------------------------------------------------------------
def camera(eye, target, fov_y_degrees, aspect):
    """a perspective camera as (eye, right, up, forward, tan half fov x, tan half fov y); the ray through ndc (a, b) is forward + a tx right + b ty up"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    ty = np.tan(np.radians(fov_y_degrees) / 2)
    return eye, right, up, fwd, ty * aspect, ty


def world_to_clip(cam):
    """row-major float32 4 x 4: clip.x = dot(P - eye, right) / tx, clip.y = dot(P - eye, up) / ty, clip.z = clip.w = dot(P - eye, forward) -- the inverse of the
    ray above, ndc = clip.xy / clip.w, no y flip"""
    eye, right, up, fwd, tx, ty = cam
    M = np.zeros((4, 4))
    for r, v in ((0, right / tx), (1, up / ty), (2, fwd), (3, fwd)):
        M[r, :3], M[r, 3] = v, -np.dot(v, eye)
    return M.astype(np.float32).reshape(16)


BOX = (np.array([-1.6, 0.0, -2.6]), np.array([-0.4, 1.2, -1.6]))
SPHERE = (np.array([0.9, 0.6, -1.8]), 0.6)
WALL_Z, WALL_TOP = -4.0, 2.4
ALBEDOS = np.array([[0.7, 0.7, 0.7], [0.6, 0.3, 0.2], [0.2, 0.5, 0.3], [0.3, 0.3, 0.8]])


def cast(cam, width, height):
    """first hits of the pixel centres' rays, float64, rounded once: a floor (instance 0), a back wall of finite height (1), a box (2), a sphere (3, kind 2); a miss
    above the wall -> ids uint32, normal, position, albedo float32, (h, w, 4) each, in skh_render_aovs' layout"""
    eye, right, up, fwd, tx, ty = cam
    h, w = height, width
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b = (xx + 0.5) / w * 2 - 1, (yy + 0.5) / h * 2 - 1
    D = fwd + (a * tx)[..., None] * right + (b * ty)[..., None] * up
    t = np.full((h, w), np.inf)
    inst = np.full((h, w), -1)
    Nn = np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        def take(tc, ok, i, n):
            nonlocal t, inst, Nn
            ok = ok & (tc > 1e-9) & (tc < t)
            t, inst = np.where(ok, tc, t), np.where(ok, i, inst)
            Nn = np.where(ok[..., None], n, Nn)

        tf = -eye[1] / D[..., 1]
        take(tf, np.isfinite(tf), 0, np.array([0.0, 1.0, 0.0]))
        tw = (WALL_Z - eye[2]) / D[..., 2]
        yw = eye[1] + tw * D[..., 1]
        take(tw, np.isfinite(tw) & (yw >= 0) & (yw <= WALL_TOP), 1, np.array([0.0, 0.0, 1.0]))
        lo, hi = BOX
        t0, t1 = (lo - eye) / D, (hi - eye) / D
        tn, tfar = np.minimum(t0, t1), np.maximum(t0, t1)
        tin, tout = tn.max(-1), tfar.min(-1)
        ax = tn.argmax(-1)
        nb = np.zeros((h, w, 3))
        for k in range(3):
            nb[..., k] = np.where(ax == k, -np.sign(D[..., k]), 0.0)
        take(tin, tin <= tout, 2, nb)
        cs, rs_ = SPHERE
        oc = eye - cs
        A, B, Cq = (D * D).sum(-1), 2 * (D * oc).sum(-1), (oc * oc).sum() - rs_ * rs_
        disc = B * B - 4 * A * Cq
        ts = (-B - np.sqrt(disc)) / (2 * A)
        Ps = eye + ts[..., None] * D
        take(ts, disc > 0, 3, (Ps - cs) / rs_)
    hit = inst >= 0
    Pw = np.where(hit[..., None], eye + np.where(hit, t, 0.0)[..., None] * D, 0.0)
    ids = np.zeros((h, w, 4), np.uint32)
    ids[..., 0] = np.where(hit, inst, 0xFFFFFFFF)
    ids[..., 1] = np.where(hit, 0, 0xFFFFFFFF)
    ids[..., 2] = np.where(hit, inst, 0xFFFFFFFF)
    ids[..., 3] = np.where(hit, np.where(inst == 3, 2, 1), 0)
    Nf, Pf, Af = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    Nf[..., :3], Nf[..., 3] = Nn, np.where(hit, 1.0, 0.0)
    Pf[..., :3], Pf[..., 3] = Pw, np.where(hit, 1.0, 0.0)
    alb = ALBEDOS[np.clip(inst, 0, 3)]
    checker = ((np.floor(Pw[..., 0] * 2) + np.floor(Pw[..., 2] * 2)) % 2 == 0) & (inst == 0)
    alb = np.where(checker[..., None], [0.9, 0.9, 0.9], alb)
    alb = np.where(((inst == 1) & (Pw[..., 0] > 1.0))[..., None], [0.0, 0.01, 0.2], alb)  # (below, below and above the floor of 0.05)
    Af[..., :3], Af[..., 3] = np.where(hit[..., None], alb, 0.0), np.where(hit, 1.0, 0.0)
    return ids, Nf, Pf, Af


def plant(ids, N, P, A, rect, kind):
    """a planted rectangle (y0, y1, x0, x1) of kind 0 (a miss) or 3 (a light proxy), with the words skh_render_aovs gives them"""
    y0, y1, x0, x1 = rect
    ids[y0:y1, x0:x1, 3] = kind
    if kind == 0:
        ids[y0:y1, x0:x1, :3] = 0xFFFFFFFF
        N[y0:y1, x0:x1], P[y0:y1, x0:x1], A[y0:y1, x0:x1] = 0.0, 0.0, 0.0
    else:
        ids[y0:y1, x0:x1, 2] = 0xFFFFFFFF
        N[y0:y1, x0:x1] = 0.0
        A[y0:y1, x0:x1] = 1.0


def synthetic(width=67, height=45, seed=5):
    """two perspective cameras a large step apart over the scene of cast().  -> {"color", "ids", "normal", "position", "albedo"} of the current frame, "prev":
    {"history", "ids", "normal", "position"}, "matrix" (the previous camera's world_to_clip), "params" (a record for them).  The colour and the previous history are
    noisy; a NaN pixel, a miss rectangle and a light-proxy rectangle are planted in each frame; the history lengths are mixed and include 0 and a fraction.
    Images smaller than 24 x 24 get no planted pixels."""
    rs = np.random.RandomState(seed)
    h, w = height, width
    aspect = w / float(h)
    cam_prev = camera((0.0, 1.2, 2.0), (0.0, 0.6, -2.0), 55.0, aspect)
    cam_now = camera((1.0, 1.5, 1.7), (-0.3, 0.5, -2.0), 55.0, aspect)
    ids, N, P, A = cast(cam_now, w, h)
    pids, pN, pP, pA = cast(cam_prev, w, h)
    big = h >= 24 and w >= 24
    if big:
        plant(ids, N, P, A, (h // 2, h // 2 + 3, 4, 12), 0)
        plant(ids, N, P, A, (h // 2 + 5, h // 2 + 8, w - 14, w - 6), 3)
        plant(pids, pN, pP, pA, (h - 8, h - 5, w // 2, w // 2 + 7), 0)
        plant(pids, pN, pP, pA, (h // 3, h // 3 + 3, w // 3, w // 3 + 6), 3)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    irr = 0.6 + 0.3 * np.sin(xx * 0.11) * np.cos(yy * 0.07)
    C = np.zeros((h, w, 4), np.float32)
    C[..., :3] = A[..., :3] * (irr[..., None] + rs.uniform(-0.4, 0.4, (h, w, 3)))
    C[..., 3] = rs.uniform(0.0, 1.0, (h, w))
    C[ids[..., 3] == 3, :3] = 40.0
    Hs = np.zeros((h, w, 4), np.float32)
    Hs[..., :3] = irr[..., None] + rs.uniform(-0.2, 0.2, (h, w, 3))
    Hs[..., 3] = rs.choice([1.0, 2.0, 5.0, 17.5, 32.0, 8.0], size=(h, w))
    Hs[rs.uniform(size=(h, w)) < 0.03, 3] = 0.0  # (a pixel whose history a previous call dropped: never a tap)
    psurf = (pids[..., 3] == 1) | (pids[..., 3] == 2)
    Hs[~psurf] = 0.0  # (what a previous call wrote there)
    if big:
        C[..., 3].view(np.uint32)[0, :8] = [0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000, 0xDEADBEEF, 0x7FBFFFFF]
        C[h - 6, 9, 0] = np.nan
        C[7, w - 9, 1] = np.inf
        Hs[h - 10, w // 2 - 6, 1] = np.nan
        Hs[h - 12, w // 3, 3] = np.nan
        Hs[h - 4, 5, 2] = np.inf
    M = world_to_clip(cam_prev)
    return {"color": C, "ids": ids, "normal": N, "position": P, "albedo": A, "prev": {"history": Hs, "ids": pids, "normal": pN, "position": pP}, "matrix": M,
            "params": params(w, h, M)}
