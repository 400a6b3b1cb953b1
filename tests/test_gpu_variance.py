"""Variance guidance on the device (skh_moments, skh_denoise_variance; DESIGN.md section 2, "Variance guidance").  skh_moments has no transcendental and must
give the bits of tests/varianceref.py's moments32; its float64 twin with a written-out bar is the second yardstick.  The filter is held, level by level and from
the device's own input to each level, to level64's bar with no pixel excluded, to skh_denoise's bits where the luminance term is off, and to three closed forms
that show the variance, and nothing else, opening and closing the stop.  Every test calls a new entry point, so each fails without the feature.

Figures on an MI355X: docs/LOG.md has the lines the tests print."""
import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import denoiseref as D
from tests import temporalref as T
from tests import varianceref as V
from tests.test_gpu_temporal import orbit, sample_frame

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 300), (300, 1), (64, 64), (65, 63), (67, 45)]
INF = float("inf")
U = V.U


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    from strelka_amd import build, capi

    build.build()
    c = capi.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_moments
# ---------------------------------------------------------------------------------------------------------------------------------------------
def moments_case(ctx, s, p, prev, label):
    motion, pm = (s["motion"], s["prev_moments"]) if prev else (None, None)
    args = (s["color"], s["ids"], s["position"], s["albedo"], motion, pm, p)
    got = ctx.moments(s["color"], s, motion, pm, p)
    want, ref = V.moments32(*args), V.moments64(*args)
    differing = int((bits(got) != bits(want)).any(axis=-1).sum())
    ratio = V.check_moments(got, ref)
    surf = ref["surface"]
    print(f"{label}: pixels that differ from the float32 restatement {differing} of {got.shape[0] * got.shape[1]}; worst error / float64 bar {ratio:.3f} over "
          f"{int((surf & ~ref['ambiguous']).sum())} unambiguous of {int(surf.sum())} surface pixels")
    assert np.array_equal(bits(got), bits(want)), label
    assert ratio <= 1.0 and ref["ambiguous"].sum() <= max(1, 0.02 * surf.sum())
    return got, ref


@pytest.mark.parametrize("prev", [True, False])
@pytest.mark.parametrize("flags", [T.DEMODULATE, 0])
def test_moments_synthetic_bit_for_bit_and_inside_the_bar(ctx, flags, prev):
    s = V.synthetic_moments()
    p = np.array(s["params"])
    p["flags"] = flags
    got, ref = moments_case(ctx, s, p, prev, f"67 x 45, flags {flags}, {'a' if prev else 'no'} previous frame")
    surf = ref["surface"]
    if prev:
        used = ref["used"][surf]
        assert (used == 4).mean() > 0.3 and (used == 0).mean() > 0.05 and ((used > 0) & (used < 4)).sum() > 50
        assert (got[surf][:, 3] > 1.0).mean() > 0.5
    else:
        assert (got[surf][:, 3] == 1.0).all() and np.array_equal(got[surf][:, 1], got[surf][:, 0] * got[surf][:, 0]) and not got[surf][:, 2].any()


@pytest.mark.parametrize("w,h", SHAPES[:-1])
def test_moments_shapes_bit_for_bit(ctx, w, h):
    s = V.synthetic_moments(w, h, seed=w + h)
    for prev in (True, False):
        moments_case(ctx, s, s["params"], prev, f"{w} x {h}, {'a' if prev else 'no'} previous frame")


def test_moments_mask_word(ctx):
    """a garbage mask word behaves as 0; a mask bit on a tap outside the image is ignored"""
    s = V.synthetic_moments()
    p = s["params"]
    h, w = s["ids"].shape[:2]
    zero = np.array(s["motion"])
    zero[..., 3] = 0.0
    none = ctx.moments(s["color"], s, zero, s["prev_moments"], p)
    first = ctx.moments(s["color"], s, None, None, p)
    assert np.array_equal(bits(none), bits(first))  # (no used tap: the pixel without history)
    garbage = np.array(s["motion"])
    garbage[..., 3] = np.array([np.nan, -1.0, 16.0, 1e9], np.float32)[np.arange(h) % 4][:, None]
    assert np.array_equal(bits(ctx.moments(s["color"], s, garbage, s["prev_moments"], p)), bits(none))
    # every bit set everywhere: the taps outside the image stay out (their clamped addresses hold valid records, which would be blended otherwise)
    full = np.array(s["motion"])
    full[..., 3] = 15.0
    got = ctx.moments(s["color"], s, full, s["prev_moments"], p)
    args = (s["color"], s["ids"], s["position"], s["albedo"], full, s["prev_moments"], p)
    ref = V.moments64(*args)
    assert np.array_equal(bits(got), bits(V.moments32(*args))) and V.check_moments(got, ref) <= 1.0
    yy, xx = np.mgrid[0:h, 0:w]
    ix, iy = np.floor(s["motion"][..., 0] + xx), np.floor(s["motion"][..., 1] + yy)
    projects = s["motion"][..., :3].any(-1) | (s["motion"][..., 3] != 0)
    outside = ref["surface"] & projects & ((ix < 0) | (ix + 1 >= w) | (iy < 0) | (iy + 1 >= h))
    print(f"mask 15 everywhere: {int(outside.sum())} surface pixels have a tap outside the image; used taps there: {np.bincount(ref['used'][outside], minlength=5).tolist()}")
    assert outside.sum() >= 5 and (ref["used"][outside] < 4).all()


def test_moments_refusals_write_nothing(ctx):
    from strelka_amd import capi

    s = V.synthetic_moments()
    h, w = s["ids"].shape[:2]
    names = ("color", "ids", "position", "albedo", "motion", "prev_moments")
    d = {n: ctx.buffer_alloc(16 * w * h) for n in names + ("out",)}
    try:
        for n in names:
            ctx.buffer_upload(d[n], s[n])
        good = [s["params"]] + [d[n] for n in names] + [d["out"]]
        ctx.moments_device(*good)
        before = ctx.moments_info()
        assert before["calls"] >= 1 and before["ms_last"] > 0.0
        ctx.buffer_upload(d["out"], np.full((h, w, 4), 7.25, np.float32))
        cases = {}
        for k, name in ((1, "no colour"), (2, "no ids"), (3, "no position"), (4, "no albedo under DEMODULATE"), (5, "previous moments without the motion plane"),
                        (6, "a motion plane without previous moments"), (7, "no output")):
            a = list(good)
            a[k] = None
            cases[name] = a
        alias = list(good)
        alias[7] = alias[6]
        cases["the moments written over the ones the taps read"] = alias
        for field, value in (("width", 0), ("max_history", 0.5), ("initial_length", 40.0), ("albedo_floor", 0.0), ("flags", 3)):
            q = np.array(s["params"])
            q[field] = value
            cases[field] = [q] + good[1:]
        out = np.zeros((h, w, 4), np.float32)
        for name, a in cases.items():
            with pytest.raises(capi.SkhError, match="skh_moments"):
                ctx.moments_device(*a)
            ctx.buffer_download(d["out"], out)
            assert (out == 7.25).all(), name
        ctx.buffer_download(d["prev_moments"], out)
        assert np.array_equal(bits(out), bits(s["prev_moments"]))
        after = ctx.moments_info()
        assert (after["calls"], after["pixels"]) == (before["calls"], before["pixels"])
    finally:
        for v in d.values():
            ctx.buffer_free(v)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_denoise_variance: level by level from the device's own input, the levels of one call, the estimate
# ---------------------------------------------------------------------------------------------------------------------------------------------
def check_pass_through(got, color, valid, label):
    assert np.array_equal(bits(got["image"])[..., 3], bits(color)[..., 3]), f"{label}: an alpha word changed"
    assert np.array_equal(bits(got["image"])[~valid], bits(color)[~valid]), f"{label}: a pixel that is no surface pixel changed"
    if "moments" in got:
        assert not bits(got["moments"])[~valid].any(), f"{label}: a pixel that is no surface pixel has moments"


def chain(ctx, s, w, h, sigma_luminance=4.0, epsilon=1e-2, levels=8):
    """levels 0 .. levels - 1 by one-level calls (the first demodulates; none remodulates), each held to level64's bar from the device's own input to it"""
    color, moments = s["color"], s["moments"]
    worst_c = worst_v = 0.0
    for lvl in range(levels):
        p = V.vparams(w, h, first_level=lvl, levels=1, sigma_luminance=sigma_luminance, epsilon=epsilon, flags=V.DEMODULATE if lvl == 0 else 0)
        c, v, valid = V.pack(color, s["ids"], s["albedo"], moments, p)
        got = ctx.denoise_variance(color, s, moments, p)
        check_pass_through(got, color, valid, f"level {lvl}")
        out, bar, vout, vbar = V.level64(c, v, valid, s["normal"], s["position"], lvl, p)
        rc, rv = V.worst(got["image"][..., :3], out, bar, valid), V.worst(got["moments"][..., 2], vout, vbar, valid)
        assert rc <= 1.0 and rv <= 1.0, (lvl, rc, rv)
        assert np.array_equal(bits(got["moments"])[valid][:, [0, 1, 3]], bits(s["moments"])[valid][:, [0, 1, 3]]), lvl  # mu1, mu2, nm: copies
        worst_c, worst_v = max(worst_c, rc), max(worst_v, rv)
        color, moments = got["image"], got["moments"]
    return color, moments, worst_c, worst_v


@pytest.mark.parametrize("w,h", SHAPES)
def test_levels_inside_the_bar_and_one_call_equals_the_chain(ctx, w, h):
    s = V.synthetic(w, h, seed=w + h)
    color, moments, rc, rv = chain(ctx, s, w, h)
    whole = ctx.denoise_variance(s["color"], s, s["moments"], V.vparams(w, h, levels=8, flags=V.DEMODULATE))
    print(f"{w} x {h}, levels 0 .. 7 from the device's own input: worst error / bar: colour {rc:.3f}, variance {rv:.3f}")
    assert np.array_equal(bits(whole["image"]), bits(color)) and np.array_equal(bits(whole["moments"]), bits(moments))
    # ... and with the last call remodulating
    tail = ctx.denoise_variance(s["color"], s, s["moments"], V.vparams(w, h, levels=8, flags=V.DEMODULATE | V.REMODULATE))
    valid = D.surface_mask(s["color"], s["ids"])
    m = D.modulation(s["albedo"], 0.05)
    assert np.array_equal(bits(tail["image"][..., :3])[valid], bits(color[..., :3] * m)[valid]) and np.array_equal(bits(tail["moments"]), bits(moments))
    check_pass_through(tail, s["color"], valid, "remodulated")


@pytest.mark.parametrize("w,h", [(1, 1), (64, 64), (65, 63), (67, 45)])
def test_estimate_against_estimate64(ctx, w, h):
    """level 7 alone on an image smaller than its step is the centre tap alone: v_out = ((w w) v0) / (sw sw) with w = sw = 9/64 exactly, v0 within the level's
    53 u of what the pack pass computed"""
    s = V.synthetic(w, h, seed=w + h)
    for min_history in (4.0, 12.0):
        p = V.vparams(w, h, first_level=7, levels=1, min_history=min_history, flags=V.DEMODULATE | V.ESTIMATE)
        c, v0, valid = V.pack(s["color"], s["ids"], s["albedo"], s["moments"], p)
        v, bar = V.estimate64(v0, valid, s["normal"], s["position"], s["moments"], p)
        got = ctx.denoise_variance(s["color"], s, s["moments"], p)
        check_pass_through(got, s["color"], valid, "estimate")
        ratio = V.worst(got["moments"][..., 2], v, bar + V.K_VAR * U * v, valid)
        with np.errstate(invalid="ignore"):
            young = valid & ~(s["moments"][..., 3] >= min_history)
        print(f"{w} x {h}, min_history {min_history}: {int(young.sum())} of {int(valid.sum())} surface pixels take the 7 x 7 estimate; worst error / bar {ratio:.3f}")
        assert ratio <= 1.0
        # (one tap: the colour is (w c) / w -- a product and a quotient, one u spare)
        assert (np.abs(got["image"][..., :3].astype(np.float64) - c)[valid] <= 3 * U * np.abs(c.astype(np.float64))[valid]).all()
        plain = ctx.denoise_variance(s["color"], s, s["moments"], V.vparams(w, h, first_level=7, levels=1, min_history=min_history, flags=V.DEMODULATE))
        if young.any() and w > 1:
            assert not np.array_equal(bits(plain["moments"][..., 2])[young], bits(got["moments"][..., 2])[young])
        assert np.array_equal(bits(plain["moments"])[valid & ~young], bits(got["moments"])[valid & ~young])


def test_in_place_aliases_and_no_moments_output(ctx):
    s = V.synthetic()
    h, w = s["ids"].shape[:2]
    p = V.vparams(w, h, levels=4, flags=7)
    want = ctx.denoise_variance(s["color"], s, s["moments"], p)
    names = ("color", "ids", "normal", "position", "albedo", "moments")
    d = {n: ctx.buffer_alloc(16 * w * h) for n in names + ("out", "mout")}
    out = np.zeros((h, w, 4), np.float32)

    def down(n):
        ctx.buffer_download(d[n], out)
        return out.copy()

    try:
        for n in names:
            ctx.buffer_upload(d[n], s[n])
        a = [p] + [d[n] for n in names]
        # d_moments_out == NULL: the colour keeps its bits, nothing else is written
        ctx.buffer_upload(d["mout"], np.full((h, w, 4), 7.25, np.float32))
        ctx.denoise_variance_device(*a, d["out"], None)
        assert np.array_equal(bits(down("out")), bits(want["image"])) and (down("mout") == 7.25).all()
        assert np.array_equal(bits(down("moments")), bits(s["moments"])) and np.array_equal(bits(down("color")), bits(s["color"]))
        # d_moments_out == d_moments, d_out == d_color
        ctx.denoise_variance_device(*a, d["color"], d["moments"])
        assert np.array_equal(bits(down("color")), bits(want["image"])) and np.array_equal(bits(down("moments")), bits(want["moments"]))
        info, dn = ctx.vdenoise_info(), ctx.denoise_info()
        assert info["scratch_bytes"] == dn["scratch_bytes"] and 56 * w * h <= info["scratch_bytes"] <= 2 * 56 * w * h + 4 * 4096 and info["ms_last"] > 0.0
        ctx.denoise_variance_device(None, None, None, None, None, None, None, None, None)
        assert ctx.vdenoise_info()["scratch_bytes"] == 0 and ctx.denoise_info()["scratch_bytes"] == 0
    finally:
        for v in d.values():
            ctx.buffer_free(v)


def test_vdenoise_refusals_write_nothing(ctx):
    from strelka_amd import capi

    s = V.synthetic()
    h, w = s["ids"].shape[:2]
    names = ("color", "ids", "normal", "position", "albedo", "moments")
    d = {n: ctx.buffer_alloc(16 * w * h) for n in names + ("out", "mout")}
    try:
        for n in names:
            ctx.buffer_upload(d[n], s[n])
        for n in ("out", "mout"):
            ctx.buffer_upload(d[n], np.full((h, w, 4), 7.25, np.float32))
        good = [V.vparams(w, h, levels=2, flags=7)] + [d[n] for n in names] + [d["out"], d["mout"]]
        ctx.denoise_variance_device(*good[:7], d["color"], None)  # (so that there is a previous state: the counters)
        ctx.buffer_upload(d["color"], s["color"])
        before = ctx.vdenoise_info()
        cases = {}
        for k, name in ((1, "no colour"), (2, "no ids"), (3, "no normal"), (4, "no position"), (5, "no albedo under a modulation flag"), (6, "no moments"), (7, "no output")):
            a = list(good)
            a[k] = None
            cases[name] = a
        for field, value in (("width", 0), ("levels", 9), ("sigma_luminance", 0.0), ("sigma_luminance", np.nan), ("sigma_normal", -1.0), ("albedo_floor", INF),
                             ("epsilon", 0.0), ("epsilon", INF), ("min_history", 0.5), ("min_history", np.nan), ("flags", 8)):
            q = np.array(good[0])
            q[field] = value
            assert not capi.vdenoise_check(q)
            cases[f"{field} {value}"] = [q] + good[1:]
        out = np.zeros((h, w, 4), np.float32)
        for name, a in cases.items():
            with pytest.raises(capi.SkhError, match="skh_denoise_variance"):
                ctx.denoise_variance_device(*a)
            for n in ("out", "mout"):
                ctx.buffer_download(d[n], out)
                assert (out == 7.25).all(), (name, n)
        after = ctx.vdenoise_info()
        assert (after["calls"], after["pixels"]) == (before["calls"], before["pixels"]) and before["calls"] >= 1
    finally:
        for v in d.values():
            ctx.buffer_free(v)


@pytest.mark.parametrize("w,h", SHAPES)
def test_luminance_term_off_is_skh_denoise_with_the_colour_term_off(ctx, w, h):
    """sigma_luminance = +inf against skh_denoise with sigma_color = +inf: a = (0 + tn) + tp on both sides, so the colour output has the same bits"""
    s = V.synthetic(w, h, seed=w + h)
    for flags in (3, 0):
        got = ctx.denoise_variance(s["color"], s, s["moments"], V.vparams(w, h, levels=5, sigma_luminance=INF, flags=flags | V.ESTIMATE))
        want = ctx.denoise(s["color"], s, D.params(w, h, levels=5, sigma_color=INF, flags=flags))
        assert np.array_equal(bits(got["image"]), bits(want)), (w, h, flags)
    valid = D.surface_mask(s["color"], s["ids"])
    if valid.sum() > 100:
        on = ctx.denoise_variance(s["color"], s, s["moments"], V.vparams(w, h, levels=5, sigma_luminance=4.0, flags=3))
        assert not np.array_equal(bits(on["image"]), bits(want))  # (the term does something when it is on)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------------------------------------------------------------------------
def flat(n, rgb, variance):
    """an n x n flat plane seen head-on, one material; rgb (n, n, 3) or a triple; MOMENTS with the given variance and a long history"""
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    s = {k: np.zeros((n, n, 4), np.float32) for k in ("color", "normal", "position", "albedo", "moments")}
    s["ids"] = np.zeros((n, n, 4), np.uint32)
    s["ids"][..., 3] = 1
    s["normal"][..., 2] = 1.0
    s["position"][..., 0], s["position"][..., 1] = x * 0.1, y * 0.1
    s["albedo"][...] = 1.0
    s["color"][..., :3], s["color"][..., 3] = rgb, 1.0
    s["moments"][..., 2], s["moments"][..., 3] = variance, 32.0
    return s


def test_uniform_variance_shrinks_by_the_kernels_energy(ctx):
    """a constant image, flat guides, uniform variance v: every weight is h[dx] h[dy] (tl = tn = tp = 0, exp(0) = 1), so at an interior pixel the colour is unchanged
    and v_out = v sum (h h)^2 = v (70/256)^2.  The weights and their squares are dyadic and exact; the 25 products with v and the 24 additions round: 49 u."""
    n, v = 9, 0.37
    s = flat(n, (0.5, 0.25, 1.0), v)
    got = ctx.denoise_variance(s["color"], s, s["moments"], V.vparams(n, n, levels=1, sigma_luminance=4.0, epsilon=1e-2))
    inner = (slice(2, n - 2), slice(2, n - 2))
    want = float(np.float32(v)) * (70.0 / 256.0) ** 2
    err = np.abs(got["moments"][inner][..., 2].astype(np.float64) / want - 1.0).max()
    print(f"uniform variance {v}: v_out / (v (70/256)^2) - 1 = {err / U:.2f} u at the worst interior pixel")
    assert err <= 49 * U
    assert np.array_equal(bits(got["image"][inner]), bits(s["color"][inner]))


def edge(n):
    y, x = np.mgrid[0:n, 0:n]
    return np.where((x < n // 2)[..., None], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]).astype(np.float32)  # (the coefficients of lum sum to 1 within 2 u)


def test_a_noise_free_edge_stays_closed(ctx):
    """luminance 1 | 2 with v = 0, epsilon 1e-3: across the edge tl = 1000, a clamps to 64, and e^-64 weighs nothing"""
    n = 24
    s = flat(n, edge(n), 0.0)
    got = ctx.denoise_variance(s["color"], s, s["moments"], V.vparams(n, n, levels=5, sigma_luminance=4.0, epsilon=1e-3))
    moved = np.abs(got["image"][..., :3].astype(np.float64) - s["color"][..., :3]).max()
    print(f"step edge without variance: the largest change of a pixel over five levels {moved:.2e}")
    assert moved <= 1e-6 and not got["moments"][..., 2].any()


def test_variance_opens_the_edge(ctx):
    """the same image with v = 1, sigma_luminance = 4: tl = 1 / (4 + 1e-3) across the edge, and the two columns at it move toward each other.  The exact value is
    level64's; the device lies inside its bar"""
    n = 24
    s = flat(n, edge(n), 1.0)
    p = V.vparams(n, n, levels=1, sigma_luminance=4.0, epsilon=1e-3)
    got = ctx.denoise_variance(s["color"], s, s["moments"], p)
    c, v, valid = V.pack(s["color"], s["ids"], None, s["moments"], p)
    out, bar, vout, vbar = V.level64(c, v, valid, s["normal"], s["position"], 0, p)
    assert V.worst(got["image"][..., :3], out, bar, valid) <= 1.0 and V.worst(got["moments"][..., 2], vout, vbar, valid) <= 1.0
    row = n // 2
    left, right = out[row, n // 2 - 1, 0], out[row, n // 2, 0]
    # the closed form at an interior row: the taps two and one column across the edge weigh h e^-tl against h on the own side
    e = np.exp(-1.0 / (4.0 + float(np.float32(1e-3))))
    h = D.H5
    assert abs(left - (h[0] + h[1] + h[2] + (h[3] + h[4]) * e * 2.0) / (h[0] + h[1] + h[2] + (h[3] + h[4]) * e)) < 1e-6
    print(f"step edge with variance 1: the columns at the edge go from 1 | 2 to {left:.5f} | {right:.5f}; device {got['image'][row, n // 2 - 1, 0]:.5f} | {got['image'][row, n // 2, 0]:.5f}")
    assert left - 1.0 > 0.05 and 2.0 - right > 0.05
    assert got["image"][row, n // 2 - 1, 0] - 1.0 > 0.05 and 2.0 - got["image"][row, n // 2, 0] > 0.05


# ---------------------------------------------------------------------------------------------------------------------------------------------
# quality: the orbit of tests/test_gpu_temporal.py
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_an_orbit_of_twelve_poses_guided_is_below_temporal_alone():
    """measured on an MI355X (rms error against 1024 spp): temporal 0.02102; temporal then skh_denoise 0.01985; guided at sigma_luminance 0.125: 0.01999, 0.25: 0.02005,
    0.5: 0.02331, 1: 0.02868, 2: 0.03221, 4: 0.03381, 8: 0.03489.  None of 1, 2, 4, 8 is below temporal alone: the per-sample variance has a heavy tail (median
    0.0047, 99.9th percentile 2.2), and a pixel with a bright sample in its history opens the stop for every pixel its variance is filtered into (with the variance
    capped at its 90th percentile, sigma_luminance 1 gives 0.01947).  The default is 0.25."""
    from strelka_amd import capi

    W = H = 128
    POSES, STEP = 12, 1.0
    sc = scenes.cornell_box()
    arr = sc.arrays()
    c, truth = capi.Context(0), capi.Context(0)
    try:
        for x in (c, truth):
            x.set_scene(arr)
            x.resize(W, H)
        d_image = c.buffer_alloc(16 * W * H)
        prev = prev_aov = moments = None
        for k in range(POSES):
            cam = orbit(sc.getCamera(), STEP * k)
            aov = S.aov_params(cam, W, H)
            guides = c.render_guides(aov)
            raw = sample_frame(c, cam, W, H, k, d_image)
            tp = S.temporal_params(W, H, prev_aov, scene=arr)
            out = c.temporal(raw, guides, prev, tp)
            moments = c.moments(raw, guides, out["motion"] if prev is not None else None, moments, tp)
            prev = {"history": out["history"], "ids": guides["ids"], "normal": guides["normal"], "position": guides["position"]}
            prev_aov = aov
        c.buffer_free(d_image)
        truth.render_subframes(S.frame_params(cam, W, H, subframe_index=0, spp_total=1024, max_depth=4), 1024)
        want = truth.read_accum()[..., :3].astype(np.float64)
        kind = guides["ids"][..., 3]
        surf = ((kind == 1) | (kind == 2)) & np.isfinite(raw[..., :3]).all(-1)
        rms = lambda img: float(np.sqrt(((img[..., :3].astype(np.float64) - want)[surf] ** 2).mean()))
        e_temporal = rms(out["image"])
        e_plain = rms(c.denoise(out["image"], guides, S.denoise_params(W, H, scene=arr, image=out["image"], guides=guides)))
        table = {}
        for sigma in (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
            vp = S.vdenoise_params(W, H, sigma_luminance=sigma, scene=arr, image=out["image"], guides=guides)
            table[sigma] = rms(c.denoise_variance(out["image"], guides, moments, vp, moments_out=False)["image"])
        default = rms(c.denoise_variance(out["image"], guides, moments, S.vdenoise_params(W, H, scene=arr, image=out["image"], guides=guides), moments_out=False)["image"])
        nm, var = moments[..., 3][surf], moments[..., 2][surf]
        print(f"cornell box {W} x {H}, pose {POSES} of an orbit in steps of {STEP} degrees, one sample per pose; rms error against 1024 spp over the surface pixels: "
              f"temporal {e_temporal:.5f}, temporal then skh_denoise {e_plain:.5f}, temporal + moments then skh_denoise_variance at sigma_luminance "
              + ", ".join(f"{k:g}: {v:.5f}" for k, v in table.items()) + f"; at the default ({S.VDENOISE_SIGMA_LUMINANCE:g}) {default:.5f}, "
              f"{default / e_plain:.3f} of skh_denoise's and {default / e_temporal:.3f} of temporal alone; moments' length: mean {nm.mean():.2f}, below 4: {float((nm < 4).mean()):.3f}; "
              f"mean standard deviation {float(np.sqrt(var).mean()):.4f}")
        assert default < e_temporal
    finally:
        c.close(), truth.close()
