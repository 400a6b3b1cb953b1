"""The denoiser off the GPU ("Denoiser"): the ABI's symbols and the records' layout through the C compiler; skh_denoise_check's accept / refuse
table; the closed forms of the definition in tests/denoiseref.py; a float32 evaluation of the definition, operation by operation, against the reference's error bar;
scene.denoise_params; and HipRender's parameter mapping through a stand-alone program (tests/cpp/hipdenoise_params_main.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import build, capi, scene as S
from tests import denoiseref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# header <-> library <-> binding
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_layout(lib, tmp_path):
    for name in ("skh_denoise_check", "skh_denoise", "skh_get_denoise_info", "skh_buffer_upload"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    for method in ("denoise", "denoise_device", "denoise_info", "render_guides", "buffer_upload"):
        assert callable(getattr(capi.Context, method))
    dt = S.DENOISE_PARAMS
    fields = ("width", "height", "first_level", "levels", "sigma_color", "sigma_normal", "sigma_plane", "albedo_floor", "flags", "reserved")
    assert dt.itemsize == 64 and dt.names == fields
    assert [dt.fields[n][1] for n in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]
    info = ("calls", "pixels", "ms_last", "scratch_bytes")
    assert capi.DENOISE_INFO.itemsize == 32 and capi.DENOISE_INFO.names == info and [capi.DENOISE_INFO.fields[n][1] for n in info] == [0, 8, 16, 24]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu", sizeof(skh_denoise_params), sizeof(skh_denoise_info));\n'
                   + "".join(f'printf(" %zu", offsetof(skh_denoise_params, {f}));\n' for f in fields) + "".join(f'printf(" %zu", offsetof(skh_denoise_info, {f}));\n' for f in info)
                   + 'printf(" %u %u %u\\n", SKH_DENOISE_DEMODULATE, SKH_DENOISE_REMODULATE, SKH_DENOISE_MAX_LEVEL); return SKH_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0  # SKH_ABI_VERSION == 5: the ABI grew, it did not change
    assert out.stdout.split() == [b"64", b"32"] + [str(dt.fields[n][1]).encode() for n in fields] + [b"0", b"8", b"16", b"24", b"1", b"2", b"8"]
    assert (S.DENOISE_DEMODULATE, S.DENOISE_REMODULATE, S.DENOISE_MAX_LEVEL) == (1, 2, 8) == (R.DEMODULATE, R.REMODULATE, 8)
    assert "skh_denoise.h" in [os.path.basename(d) for d in build.DEPS]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_denoise_check
# ---------------------------------------------------------------------------------------------------------------------------------------------
def good(**kw):
    args = dict(width=67, height=45, levels=5, sigma_color=0.5, sigma_normal=0.3, sigma_plane=0.05)
    args.update(kw)
    return S.denoise_params(args.pop("width"), args.pop("height"), **args)


def edited(field, value, index=None, **kw):
    p = good(**kw)
    if index is None:
        p[field] = value
    else:
        p[field][index] = value
    return p


ACCEPTED = {"the defaults": good(), "one pixel": good(width=1, height=1), "2^26 pixels": good(width=1 << 13, height=1 << 13), "2^26 in a row": good(width=1 << 26, height=1),
            "level 7 alone": good(first_level=7, levels=1), "eight levels": good(levels=8), "no flag": good(demodulate=False, remodulate=False),
            "demodulate alone": good(remodulate=False), "remodulate alone": good(demodulate=False),
            "sigma_color +inf": good(sigma_color=INF), "sigma_normal +inf": good(sigma_normal=INF), "sigma_plane +inf": good(sigma_plane=INF),
            "a tiny sigma": good(sigma_plane=1e-30), "a tiny floor": good(albedo_floor=1e-30)}
REFUSED = {"zero width": good(width=0), "zero height": good(height=0), "2^26 + 2^13 pixels": good(width=(1 << 13) + 1, height=1 << 13),
           "a product that wraps 32 bits": good(width=1 << 16, height=1 << 16), "levels 0": good(levels=0), "nine levels": good(levels=9),
           "first_level 8": good(first_level=8, levels=1), "first_level 4 + 5 levels": good(first_level=4, levels=5), "levels that wrap": good(first_level=2, levels=0xFFFFFFFF),
           "first_level that wraps": good(first_level=0xFFFFFFFF, levels=2),
           "sigma_color 0": good(sigma_color=0.0), "sigma_color < 0": good(sigma_color=-1.0), "sigma_color nan": good(sigma_color=np.nan), "sigma_color -inf": good(sigma_color=-INF),
           "sigma_normal 0": good(sigma_normal=0.0), "sigma_normal nan": good(sigma_normal=np.nan), "sigma_plane -0": good(sigma_plane=-0.0), "sigma_plane nan": good(sigma_plane=np.nan),
           "floor 0": good(albedo_floor=0.0), "floor < 0": good(albedo_floor=-0.1), "floor inf": good(albedo_floor=INF), "floor nan": good(albedo_floor=np.nan),
           "flag bit 2": edited("flags", 4), "flag bit 31": edited("flags", 0x80000003), "reserved[0]": edited("reserved", 1, 0), "reserved[6]": edited("reserved", 9, 6)}


def test_denoise_check_accepts_and_refuses(lib):
    for name, p in ACCEPTED.items():
        assert capi.denoise_check(p), name
    for name, p in REFUSED.items():
        assert not capi.denoise_check(p), name
        assert lib.skh_denoise_check(p.ctypes.data_as(C.c_void_p)) == 3, name
    assert lib.skh_denoise_check(None) == 3
    # without a context the entry points refuse instead of crashing
    assert lib.skh_denoise(None, None, None, None, None, None, None, None) == 3 and lib.skh_get_denoise_info(None, None) == 3
    assert lib.skh_buffer_upload(None, None, None, 0) == 3


def test_denoise_params_round_trip():
    from strelka_amd import scenes

    p = S.denoise_params(640, 360, levels=3, sigma_color=2.5, sigma_normal=0.25, sigma_plane=0.125, first_level=2, albedo_floor=0.0625, remodulate=False)
    assert [int(p[k]) for k in ("width", "height", "first_level", "levels", "flags")] == [640, 360, 2, 3, S.DENOISE_DEMODULATE]
    assert [float(p[k]) for k in ("sigma_color", "sigma_normal", "sigma_plane", "albedo_floor")] == [2.5, 0.25, 0.125, 0.0625] and not p["reserved"].any()
    q = np.frombuffer(p.tobytes(), S.DENOISE_PARAMS)[0]
    assert q.tobytes() == p.tobytes() and capi.denoise_check(q)
    # the defaults: five levels from 0, both flags, sigma_color = the radiance of mid-grey under the exposure, sigma_plane a fraction of the scene's diagonal
    arr = scenes.cornell_box().arrays()
    d = S.denoise_params(96, 72, scene=arr)
    assert (int(d["levels"]), int(d["first_level"]), int(d["flags"])) == (5, 0, 3) and float(d["sigma_normal"]) == np.float32(S.DENOISE_SIGMA_NORMAL)
    assert float(d["sigma_color"]) == np.float32(1.0 / np.float64(S.default_exposure()).mean())
    assert float(S.denoise_params(8, 8, exposure=(0.5, 0.5, 0.5), sigma_plane=1.0)["sigma_color"]) == 2.0
    diag = S.scene_diagonal(arr)
    pos = arr["vertices"]["pos"]
    assert 0.5 * np.linalg.norm(pos.max(0) - pos.min(0)) < diag < 4.0 * np.linalg.norm(pos.max(0) - pos.min(0))
    assert float(d["sigma_plane"]) == np.float32(S.DENOISE_PLANE_FRACTION * diag) and capi.denoise_check(d)
    with pytest.raises(ValueError):
        S.denoise_params(8, 8)  # sigma_plane is in scene units: no scene, no default


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the definition's closed forms (float64)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def flat(n):
    """an n x n flat plane seen head-on, one material"""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    N, P = np.zeros((n, n, 3)), np.zeros((n, n, 3))
    N[..., 2] = 1.0
    P[..., 0], P[..., 1] = x * 0.1, y * 0.1
    return N, P, np.ones((n, n), bool)


def test_impulse_response_is_the_b3_spline_cascade():
    """sigma_color = +inf on a flat plane: every weight is h[dx] h[dy].  The response to one bright pixel sums to 1, has support 4 (2^n - 1) + 1 after n levels, and its
    energy sum K^2 -- the variance ratio for white noise, fully interior -- is (35/128)^2 after one level"""
    n = 253  # (a pixel 62 from the impulse has taps up to 124 from it: none of them may leave the image, or its weights are renormalised)
    N, P, valid = flat(n)
    c = np.zeros((n, n, 3))
    c[n // 2, n // 2] = 1.0
    energies = {1: ((35.0 / 128.0) ** 2, 1e-15), 2: (0.0152459, 5e-8), 3: (0.00364327, 5e-9), 4: (9.00883e-4, 5e-10)}  # (figures of six digits: half a unit of the last)
    for lv in range(5):
        c, _ = R.level(c, valid, N, P, lv, INF, 0.3, 0.05)
        k = c[..., 0]
        rows = np.nonzero(k.any(axis=1))[0]
        cols = np.nonzero(k.any(axis=0))[0]
        support = 4 * (2 ** (lv + 1) - 1) + 1
        assert (rows[-1] - rows[0] + 1, cols[-1] - cols[0] + 1) == (support, support) and support == (5, 13, 29, 61, 125)[lv]
        assert abs(k.sum() - 1.0) < 1e-13 and (k >= 0).all()
        if lv + 1 in energies:
            assert abs((k * k).sum() - energies[lv + 1][0]) <= energies[lv + 1][1], (lv, (k * k).sum())
        assert np.array_equal(c[..., 0], c[..., 1]) and np.array_equal(c[..., 0], c[..., 2])


def test_edges_without_noise_stay():
    """a crease between perpendicular normals and a depth step of 0.5 between equal normals, each side of one colour: five levels change nothing (sigma_normal 0.1,
    sigma_plane 0.01: across either edge a is clamped to 64 and the tap weighs e^-64)"""
    s = R.synthetic(special=False)
    h, w = s["ids"].shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    region = np.where(x < w // 2, np.where(y >= (2 * h) // 3, 2, 1), 3)
    c = np.stack([0.2 * region, 1.0 / region, 0.5 + 0.0 * region], -1).astype(np.float64)
    valid = np.ones((h, w), bool)
    got = c
    for lv in range(5):
        got, _ = R.level(got, valid, s["normal"][..., :3], s["position"][..., :3], lv, INF, 0.1, 0.01)
    assert np.abs(got - c).max() <= 5e-16
    # the same picture with the guide terms off is blurred across both edges
    blurred, _ = R.level(c, valid, s["normal"][..., :3], s["position"][..., :3], 0, INF, INF, INF)
    assert np.abs(blurred - c).max() > 0.01


def compose(ref, color):
    """the float32 image the definition gives: the reference's value on surface pixels, the input's bits elsewhere and in alpha"""
    out = np.array(color, np.float32)
    out[..., :3] = np.where(ref["surface"][..., None], ref["out"].astype(np.float32), out[..., :3])
    return out


def test_pass_through_and_the_nan_pixel():
    """miss and light bands come back bit-equal, one NaN pixel stays one NaN pixel, one Inf pixel one Inf pixel"""
    s = R.synthetic()
    h, w = s["ids"].shape[:2]
    p = R.params(w, h, levels=5, flags=3)
    ref = R.denoise(s["color"], s["ids"], s["normal"], s["position"], s["albedo"], p)
    out = compose(ref, s["color"])
    kind = s["ids"][..., 3]
    assert (kind == 0).sum() == 42 and (kind == 3).sum() == 42 and (kind == 2).sum() == 3 * w and ref["surface"].sum() == w * h - 84 - 2
    assert R.check(out, s["color"], ref) <= 1.0  # (the bit-exact parts are asserted in there)
    bad_in, bad_out = ~np.isfinite(s["color"][..., :3]), ~np.isfinite(out[..., :3])
    assert np.array_equal(bad_in, bad_out) and bad_in.sum() == 2
    assert np.isnan(out[5, 7, 0]) and np.isinf(out[35, 50, 1])
    # the neighbours of the two were filtered, and from finite taps alone
    assert ref["surface"][5, 8] and np.isfinite(ref["out"][5, 8]).all() and not np.array_equal(out[5, 8, :3], s["color"][5, 8, :3])


def test_demodulation_keeps_the_texture():
    """a 0.9 / 0.1 checker albedo over a smooth irradiance with noise: five levels with demodulation come closer to the noise-free picture than the input is, and
    without demodulation the checker is blurred and the result is further away than the input"""
    s = R.synthetic(special=False)
    h, w = s["ids"].shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    clean = s["albedo"][..., :3].astype(np.float64) * (0.6 + 0.3 * np.sin(x * 0.11) * np.cos(y * 0.07))[..., None]
    rms = lambda a: float(np.sqrt(((a - clean) ** 2).mean()))
    args = (s["color"], s["ids"], s["normal"], s["position"], s["albedo"])
    with_demod = R.denoise(*args, R.params(w, h, levels=5, flags=3))["out"]
    without = R.denoise(*args, R.params(w, h, levels=5, flags=0, sigma_color=INF))["out"]
    e_in, e_demod, e_plain = rms(s["color"][..., :3].astype(np.float64)), rms(with_demod), rms(without)
    print(f"rms error: input {e_in:.4f}, five levels with demodulation {e_demod:.4f}, without {e_plain:.4f}")
    assert e_demod < 0.6 * e_in and e_plain > e_in


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a float32 evaluation of the definition, operation by operation, against the bar
# ---------------------------------------------------------------------------------------------------------------------------------------------
def level32(c, valid, N, P, lvl, sigma_color, sigma_normal, sigma_plane, zero_multiply=False):
    """the definition in float32 as the header writes it out: every product, sum and quotient rounded, taps in order.  exp is float64's, rounded: within half an ulp,
    inside the 1.1 ulp the bar allows skh_libm's.  zero_multiply: the form the definition forbids -- a skipped tap enters with weight 0."""
    f = np.float32
    c, N, P = (np.asarray(a, f) for a in (c, N, P))
    h, w = valid.shape
    s = 1 << lvl
    with np.errstate(all="ignore"):
        sc = f(sigma_color) * f(2.0 ** -lvl)
        kc, kn, kp = f(1.0) / (sc * sc), f(1.0) / (f(sigma_normal) * f(sigma_normal)), f(1.0) / (f(sigma_plane) * f(sigma_plane))
        yy, xx = np.mgrid[0:h, 0:w]
        sw, sx = np.zeros((h, w), f), np.zeros((h, w, 3), f)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = yy + dy * s, xx + dx * s
                inb = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.where(inb, qy, yy), np.where(inb, qx, xx)
                take = inb & valid[qy, qx]
                cq, Nq, Pq = c[qy, qx], N[qy, qx], P[qy, qx]
                e, n, g = cq - c, Nq - N, Pq - P
                tc = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) * kc
                tn = ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]) * kn
                d = (N[..., 0] * g[..., 0] + N[..., 1] * g[..., 1]) + N[..., 2] * g[..., 2]
                tp = (d * d) * kp
                a = (tc + tn) + tp
                a = np.where(a <= f(64.0), a, f(64.0))
                wq = (f(R.H5[dx + 2]) * f(R.H5[dy + 2])) * np.exp(-a.astype(np.float64)).astype(f)
                if zero_multiply:
                    wq = wq * take.astype(f)
                    sw, sx = sw + wq, sx + wq[..., None] * cq
                else:
                    sw = np.where(take, sw + wq, sw)
                    sx = np.where(take[..., None], sx + wq[..., None] * cq, sx)
        out = sx / sw[..., None]
    return np.where(valid[..., None], out, f(0.0)).astype(f)


@pytest.mark.parametrize("lvl", range(7))
def test_float32_evaluation_stays_inside_the_bar(lvl):
    s = R.synthetic()
    h, w = s["ids"].shape[:2]
    valid = R.surface_mask(s["color"], s["ids"])
    p = R.params(w, h, first_level=lvl, levels=1)
    ref = R.denoise(s["color"], s["ids"], s["normal"], s["position"], None, p)
    c = np.where(valid[..., None], s["color"][..., :3], 0.0)
    got = np.array(s["color"])
    got[..., :3] = np.where(valid[..., None], level32(c, valid, s["normal"][..., :3], s["position"][..., :3], lvl, 0.5, 0.3, 0.05), got[..., :3])
    ratio = R.check(got, s["color"], ref)
    widest = ref["bar"].max()  # (the colours are of order 1)
    print(f"level {lvl}: float32 evaluation, worst error / bar {ratio:.3f}; widest bar {widest:.2e}")
    assert ratio <= 1.0 and ratio > 0.005 and widest < 1e-5  # inside the bar, and the bar is not orders of magnitude too wide


def test_a_skipped_tap_multiplied_by_zero_poisons_the_image():
    """why the definition selects: with weight 0 x NaN in the sums, the one NaN pixel of the picture spreads over every pixel five levels reach"""
    s = R.synthetic()
    valid = R.surface_mask(s["color"], s["ids"])
    N, P = s["normal"][..., :3], s["position"][..., :3]
    good_c = bad_c = s["color"][..., :3]  # (NaN and Inf left in place on the two pixels that are not valid)
    for lv in range(5):
        good_c = np.where(valid[..., None], level32(good_c, valid, N, P, lv, INF, INF, INF), s["color"][..., :3])
        bad_c = np.where(valid[..., None], level32(bad_c, valid, N, P, lv, INF, INF, INF, zero_multiply=True), s["color"][..., :3])
    assert (~np.isfinite(good_c)).any(axis=-1).sum() == 2
    assert (~np.isfinite(bad_c)).any(axis=-1).sum() > 0.5 * valid.sum()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# oka::HipRender's parameter mapping
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_hiprender_parameter_mapping_from_a_standalone_program(lib, tmp_path):
    """tests/cpp/hipdenoise_params_main.cpp: integration/HipRender.h's hipDenoiseParams with the C header and the library alone -- the defaults are scene.py's, a
    given field is taken as it is, and what comes out passes or fails skh_denoise_check as the same record does through the binding"""
    exe = str(tmp_path / "hipdenoise_params")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "hipdenoise_params_main.cpp"),
                           "-L" + libdir, "-lstrelka_hip", "-Wl,-rpath," + libdir])
    f = np.float32
    e = S.default_exposure()
    #        levels sigmaColor sigmaNormal sigmaPlane planeFraction albedoFloor width height exposure sceneDiagonal
    cases = [(0, 0.0, 0.0, 0.0, 0.0, 0.0, 1920, 1080, e, 12.5),
             (3, 0.75, 0.125, 0.02, 0.5, 0.1, 67, 45, e, 12.5),
             (8, 0.0, 0.0, 0.0, 0.01, 0.0, 1, 1, (0.5, 0.25, 0.75), 3.0),
             (0, -1.0, -1.0, -1.0, -1.0, -1.0, 640, 360, (2.0, 2.0, 2.0), 100.0),
             (0, 0.0, 0.0, 0.0, 0.0, 0.0, 64, 64, e, 0.0),  # nothing to measure: the plane term is off
             (9, 0.0, 0.0, 0.0, 0.0, 0.0, 64, 64, e, 1.0),  # refused by the check
             (5, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 64, e, 1.0)]
    lines = ["%d %r %r %r %r %r %d %d %r %r %r %r" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], float(c[8][0]), float(c[8][1]), float(c[8][2]), c[9]) for c in cases]
    out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.decode().strip().split("\n")
    assert got[0].split() == ["64", "32"] and len(got) == 1 + len(cases)
    for c, line in zip(cases, got[1:]):
        words = line.split()
        rec = np.frombuffer(np.array([int(w, 16) for w in words[:16]], np.uint32).tobytes(), S.DENOISE_PARAMS)[0]
        ex = np.asarray(c[8], f)
        mean = f(f(f(ex[0] + ex[1]) + ex[2]) / f(3.0))
        plane = f(c[3]) if c[3] > 0 else f(f(c[4]) if c[4] > 0 else f(S.DENOISE_PLANE_FRACTION)) * f(c[9])
        want = S.denoise_params(c[6], c[7], levels=c[0] or 5, sigma_color=f(c[1]) if c[1] > 0 else f(1.0) / mean, sigma_normal=c[2] if c[2] > 0 else S.DENOISE_SIGMA_NORMAL,
                                sigma_plane=plane if plane > 0 else INF, albedo_floor=c[5] if c[5] > 0 else S.DENOISE_ALBEDO_FLOOR)
        assert rec.tobytes() == want.tobytes(), (c, rec, want)
        assert int(words[16]) == (0 if capi.denoise_check(want) else 3)
    assert [int(line.split()[16]) for line in got[1:]] == [0, 0, 0, 0, 0, 3, 3]
