"""Variance guidance off the GPU ("Variance guidance"): the ABI's symbols and the records' layout through the C compiler; the accept / refuse
tables of both checks; scene.vdenoise_params; HipRender's parameter mapping through a stand-alone program (tests/cpp/hipvariance_params_main.cpp); a float32
evaluation of one filter level against tests/varianceref.py's bar, and three one-line mutations that must leave it; moments32 against moments64's bar."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import build, capi, scene as S
from tests import varianceref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_abi_symbols_and_layout(lib, tmp_path):
    for name in ("skh_moments", "skh_get_moments_info", "skh_vdenoise_check", "skh_denoise_variance", "skh_get_vdenoise_info"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    for method in ("moments", "moments_device", "moments_info", "denoise_variance", "denoise_variance_device", "vdenoise_info"):
        assert callable(getattr(capi.Context, method))
    assert callable(capi.moments_check) and callable(capi.vdenoise_check)
    dt = S.VDENOISE_PARAMS
    fields = ("width", "height", "first_level", "levels", "sigma_luminance", "sigma_normal", "sigma_plane", "albedo_floor", "epsilon", "min_history", "flags", "reserved")
    assert dt.itemsize == 64 and dt.names == fields
    assert [dt.fields[n][1] for n in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44]
    assert capi.MOMENTS_INFO.itemsize == 24 and capi.MOMENTS_INFO.names == ("calls", "pixels", "ms_last")
    info = ("calls", "pixels", "ms_last", "scratch_bytes")
    assert capi.VDENOISE_INFO.itemsize == 32 and capi.VDENOISE_INFO.names == info
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu %zu", sizeof(skh_vdenoise_params), '
                   "sizeof(skh_vdenoise_info), sizeof(skh_moments_info));\n"
                   + "".join(f'printf(" %zu", offsetof(skh_vdenoise_params, {f}));\n' for f in fields) + "".join(f'printf(" %zu", offsetof(skh_vdenoise_info, {f}));\n' for f in info)
                   + 'printf(" %u %u %u\\n", SKH_DENOISE_DEMODULATE, SKH_DENOISE_REMODULATE, SKH_VDENOISE_ESTIMATE); return SKH_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0  # SKH_ABI_VERSION == 5: the ABI grew, it did not change
    assert out.stdout.split() == [b"64", b"32", b"24"] + [str(dt.fields[n][1]).encode() for n in fields] + [b"0", b"8", b"16", b"24", b"1", b"2", b"4"]
    assert (S.VDENOISE_ESTIMATE, V.ESTIMATE) == (4, 4)
    assert "skh_variance.h" in [os.path.basename(d) for d in build.DEPS]
    header = open(os.path.join(ROOT, "include", "strelka_hip.h")).read()
    for phrase in ("Variance guidance", "skh_moments", "skh_denoise_variance", "(0.2126f c.x + 0.7152f c.y) + 0.0722f c.z", "kl = 1 / (sigma_luminance sqrtf(vbar) + epsilon)",
                   "sv += (w w) v(q)", "v_out = sv / (sw sw)", "feeding the first level's output back into the history", "variance for a\n * still camera's accumulator"):
        assert phrase in header, phrase


def good(**kw):
    args = dict(width=67, height=45, levels=5, sigma_luminance=4.0, sigma_normal=0.3, sigma_plane=0.05, epsilon=1e-2)
    args.update(kw)
    return S.vdenoise_params(args.pop("width"), args.pop("height"), **args)


def edited(field, value, index=None, **kw):
    p = good(**kw)
    if index is None:
        p[field] = value
    else:
        p[field][index] = value
    return p


ACCEPTED = {"the defaults": good(), "one pixel": good(width=1, height=1), "2^26 pixels": good(width=1 << 13, height=1 << 13), "level 7 alone": good(first_level=7, levels=1),
            "eight levels": good(levels=8), "no flag": good(demodulate=False, remodulate=False, estimate=False), "estimate alone": good(demodulate=False, remodulate=False),
            "sigma_luminance +inf": good(sigma_luminance=INF), "sigma_normal +inf": good(sigma_normal=INF), "sigma_plane +inf": good(sigma_plane=INF),
            "a tiny epsilon": good(epsilon=1e-30), "min_history 1": good(min_history=1.0), "min_history 1e6": good(min_history=1e6)}
REFUSED = {"zero width": good(width=0), "zero height": good(height=0), "2^26 + 2^13 pixels": good(width=(1 << 13) + 1, height=1 << 13), "levels 0": good(levels=0),
           "nine levels": good(levels=9), "first_level 4 + 5 levels": good(first_level=4, levels=5), "levels that wrap": good(first_level=2, levels=0xFFFFFFFF),
           "sigma_luminance 0": good(sigma_luminance=0.0), "sigma_luminance < 0": good(sigma_luminance=-1.0), "sigma_luminance nan": good(sigma_luminance=np.nan),
           "sigma_normal 0": good(sigma_normal=0.0), "sigma_normal nan": good(sigma_normal=np.nan), "sigma_plane -0": good(sigma_plane=-0.0), "sigma_plane nan": good(sigma_plane=np.nan),
           "floor 0": good(albedo_floor=0.0), "floor inf": good(albedo_floor=INF), "floor nan": good(albedo_floor=np.nan),
           "epsilon 0": good(epsilon=0.0), "epsilon < 0": good(epsilon=-1e-3), "epsilon inf": good(epsilon=INF), "epsilon nan": good(epsilon=np.nan),
           "min_history 0.5": good(min_history=0.5), "min_history inf": good(min_history=INF), "min_history nan": good(min_history=np.nan),
           "flag bit 3": edited("flags", 8), "flag bit 31": edited("flags", 0x80000007), "reserved[0]": edited("reserved", 1, 0), "reserved[4]": edited("reserved", 9, 4)}


def test_vdenoise_check_accepts_and_refuses(lib):
    for name, p in ACCEPTED.items():
        assert capi.vdenoise_check(p), name
    for name, p in REFUSED.items():
        assert not capi.vdenoise_check(p), name
        assert lib.skh_vdenoise_check(p.ctypes.data_as(C.c_void_p)) == 3, name
    assert lib.skh_vdenoise_check(None) == 3
    # without a context the entry points refuse instead of crashing
    assert lib.skh_denoise_variance(None, None, None, None, None, None, None, None, None, None) == 3 and lib.skh_get_vdenoise_info(None, None) == 3
    assert lib.skh_moments(None, None, None, None, None, None, None, None, None) == 3 and lib.skh_get_moments_info(None, None) == 3


def test_moments_check_is_the_temporal_check():
    from tests import temporalref as T

    ok = T.params(67, 45)
    assert capi.moments_check(ok)
    for field, value in (("width", 0), ("max_history", 0.5), ("initial_length", 64.0), ("albedo_floor", 0.0), ("flags", 2), ("normal_min", 2.0), ("plane_tolerance", 0.0)):
        p = T.params(67, 45)
        p[field] = value
        assert not capi.moments_check(p) and not capi.temporal_check(p), field
    p = T.params(67, 45)
    p["prev_world_to_clip"][5] = np.nan
    assert not capi.moments_check(p)
    p = T.params(67, 45)
    p["reserved"][7] = 1
    assert not capi.moments_check(p)


def test_vdenoise_params_defaults():
    from strelka_amd import scenes

    arr = scenes.cornell_box().arrays()
    d, v = S.denoise_params(96, 72, scene=arr), S.vdenoise_params(96, 72, scene=arr)
    for k in ("width", "height", "first_level", "levels", "sigma_normal", "sigma_plane", "albedo_floor"):
        assert v[k] == d[k], k
    assert int(v["flags"]) == 7 and float(v["min_history"]) == 4.0 and float(v["sigma_luminance"]) == np.float32(S.VDENOISE_SIGMA_LUMINANCE) and not v["reserved"].any()
    assert float(v["epsilon"]) == np.float32(1e-2 / np.float64(S.default_exposure()).mean()) and capi.vdenoise_check(v)
    # with the image: a hundredth of its mean demodulated luminance over the surface pixels
    s = V.synthetic()
    c, _, valid = V.pack(s["color"], s["ids"], s["albedo"], s["moments"], V.vparams(67, 45, flags=1))
    mean = V.lum64(c.astype(np.float64))[0][valid].mean()
    e = S.vdenoise_params(67, 45, sigma_plane=0.05, image=s["color"], guides=s)["epsilon"]
    assert abs(float(e) / (1e-2 * mean) - 1.0) < 1e-6
    with pytest.raises(ValueError):
        S.vdenoise_params(8, 8)


def test_hiprender_parameter_mapping_from_a_standalone_program(lib, tmp_path):
    """tests/cpp/hipvariance_params_main.cpp: integration/HipRender.h's hipVarianceParams with the C header and the library alone"""
    exe = str(tmp_path / "hipvariance_params")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "hipvariance_params_main.cpp"),
                           "-L" + libdir, "-lstrelka_hip", "-Wl,-rpath," + libdir])
    f = np.float32
    e = tuple(float(x) for x in S.default_exposure())
    #        sigmaLuminance epsilon minHistory levels sigmaNormal sigmaPlane albedoFloor width height exposure sceneDiagonal
    cases = [(0.0, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 1920, 1080, e, 12.5),
             (2.0, 0.125, 8.0, 3, 0.125, 0.02, 0.1, 67, 45, e, 12.5),
             (-1.0, -1.0, -1.0, 8, 0.0, 0.0, 0.0, 1, 1, (0.5, 0.25, 0.75), 3.0),
             (0.0, 0.0, 0.5, 0, 0.0, 0.0, 0.0, 64, 64, e, 1.0),  # min_history < 1: refused by the check
             (0.0, 0.0, 0.0, 9, 0.0, 0.0, 0.0, 64, 64, e, 1.0)]
    lines = [" ".join(repr(float(x)) if isinstance(x, float) else str(x) for x in c[:9]) + " %r %r %r %r" % (c[9][0], c[9][1], c[9][2], c[10]) for c in cases]
    out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.decode().strip().split("\n")
    assert got[0].split() == ["64", "32", "24"] and len(got) == 1 + len(cases)
    for c, line in zip(cases, got[1:]):
        words = line.split()
        rec = np.frombuffer(np.array([int(w, 16) for w in words[:16]], np.uint32).tobytes(), S.VDENOISE_PARAMS)[0]
        ex = np.asarray(c[9], f)
        mean = f(f(f(ex[0] + ex[1]) + ex[2]) / f(3.0))
        plane = f(c[5]) if c[5] > 0 else f(S.DENOISE_PLANE_FRACTION) * f(c[10])
        want = S.vdenoise_params(c[7], c[8], levels=c[3] or 5, sigma_luminance=c[0] if c[0] > 0 else S.VDENOISE_SIGMA_LUMINANCE, sigma_normal=c[4] if c[4] > 0 else S.DENOISE_SIGMA_NORMAL,
                                 sigma_plane=plane, albedo_floor=c[6] if c[6] > 0 else S.DENOISE_ALBEDO_FLOOR, epsilon=f(c[1]) if c[1] > 0 else f(0.01) / mean,
                                 min_history=c[2] if c[2] > 0 else S.VDENOISE_MIN_HISTORY)
        assert rec.tobytes() == want.tobytes(), (c, rec, want)
        assert int(words[16]) == (0 if capi.vdenoise_check(want) else 3)
    assert [int(line.split()[16]) for line in got[1:]] == [0, 0, 0, 3, 3]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# one level in float32 against the bar, and the mutations
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packed():
    s = V.synthetic()
    h, w = s["ids"].shape[:2]
    p = V.vparams(w, h, flags=V.DEMODULATE, sigma_luminance=4.0, epsilon=1e-2)
    c, v0, valid = V.pack(s["color"], s["ids"], s["albedo"], s["moments"], p)
    return s, p, c, v0, valid


@pytest.mark.parametrize("lvl", [0, 1, 3, 6])
def test_float32_level_stays_inside_the_bar(packed, lvl):
    s, p, c, v0, valid = packed
    out, bar, vout, vbar = V.level64(c, v0, valid, s["normal"], s["position"], lvl, p)
    got, gotv = V.level32(c, v0, valid, s["normal"], s["position"], lvl, p)
    rc, rv = V.worst(got, out, bar, valid), V.worst(gotv, vout, vbar, valid)
    print(f"level {lvl}: float32 model, worst error / bar: colour {rc:.3f}, variance {rv:.3f}; widest bars {bar.max():.2e}, {(vbar / np.maximum(vout, 1e-30))[valid].max():.2e} relative")
    assert rc <= 1.0 and rv <= 1.0
    assert rc > 0.002 and rv > 0.002 and bar.max() < 1e-4  # the bars are not orders of magnitude too wide (the colours are of order 1 to 10)


@pytest.mark.parametrize("mutation", ["w_for_ww", "v_for_vbar", "no_root"])
def test_a_one_line_mutation_leaves_the_bar(packed, mutation):
    s, p, c, v0, valid = packed
    out, bar, vout, vbar = V.level64(c, v0, valid, s["normal"], s["position"], 0, p)
    got, gotv = V.level32(c, v0, valid, s["normal"], s["position"], 0, p, mutate=mutation)
    rc, rv = V.worst(got, out, bar, valid), V.worst(gotv, vout, vbar, valid)
    print(f"{mutation}: worst error / bar: colour {rc:.3g}, variance {rv:.3g}")
    assert max(rc, rv) > 100.0


def test_estimate_uses_the_young_pixels_only(packed):
    s, p, c, v0, valid = packed
    v, bar = V.estimate64(v0, valid, s["normal"], s["position"], s["moments"], p)
    nm = s["moments"][..., 3]
    with np.errstate(invalid="ignore"):
        young = valid & ~(nm >= 4.0)
    assert young.sum() > 0.15 * valid.sum() and (~young & valid).sum() > 0.5 * valid.sum()
    assert np.array_equal(v[valid & ~young], v0[valid & ~young].astype(np.float64)) and not bar[valid & ~young].any()
    assert (v[young] >= 0).all() and (v[young] > 0).mean() > 0.9 and np.isfinite(v).all()
    assert bar[young].max() < 2e-4  # (the difference e2 - e1 e1 cancels: ~100 u of second moments of order 1, times k <= 4, for a variance of order 0.01)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_moments: the float32 restatement against the float64 bar
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1])
def test_moments32_inside_moments64s_bar(flags):
    s = V.synthetic_moments()
    p = s["params"].copy()
    p["flags"] = flags
    args = (s["color"], s["ids"], s["position"], s["albedo"], s["motion"], s["prev_moments"], p)
    got, ref = V.moments32(*args), V.moments64(*args)
    surf = ref["surface"]
    assert surf.sum() > 2000 and ref["ambiguous"].sum() <= 0.02 * surf.sum()  # the reference input itself satisfies the share
    used = ref["used"][surf]
    assert (used == 0).sum() > 100 and (used == 4).sum() > 500 and ((used > 0) & (used < 4)).sum() > 50  # every branch is there
    ratio = V.check_moments(got, ref)
    print(f"flags {flags}: {surf.sum()} surface pixels, {ref['ambiguous'].sum()} ambiguous, worst error / bar {ratio:.3f}; the bar's median {np.median(ref['bar'][surf][:, :3]):.2e}, maximum {ref['bar'][..., :3].max():.2e}")
    # inside the bar, and the bar is not orders of magnitude too wide: the tap weights carry fx's error, some 67 x 4 u, and the planted previous moments differ
    # from tap to tap by about 1; the maximum belongs to grazing pixels, whose fx carries the error of a small clip.w
    assert ratio <= 1.0 and ratio > 0.005 and np.median(ref["bar"][surf][:, :3]) < 1e-4
    # without a previous frame: mu1 = l, mu2 = l l, nm = initial_length, on every surface pixel
    first = V.moments32(s["color"], s["ids"], s["position"], s["albedo"], None, None, p)
    ref0 = V.moments64(s["color"], s["ids"], s["position"], s["albedo"], None, None, p)
    assert V.check_moments(first, ref0) <= 1.0 and not ref0["ambiguous"].any()
    assert (first[surf][:, 3] == 1.0).all() and np.array_equal(first[surf][:, 1], first[surf][:, 0] * first[surf][:, 0])


def test_mask_word_garbage_is_no_tap():
    m = np.zeros((1, 8, 4), np.float32)
    m[0, :, 3] = [np.nan, -1.0, 16.0, 1e9, 15.0, 3.5, 0.0, -0.0]
    assert V.mask_of(m).tolist() == [[0, 0, 0, 0, 15, 3, 0, 0]]
