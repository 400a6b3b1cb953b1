"""History rectification off the GPU ("History rectification"): the ABI's symbols and the record's layout through the C compiler;
skh_rectify_check's table of refusals; scene.rectify_params; the conditions the synthetic input must meet; the float32 restatement (tests/rectifyref.py:
rectify32) inside the float64 reference's written-out bar, against closed forms and in a stepped sequence through temporalref's reprojection; HipRectify's
defaults through a stand-alone program.  No test here needs a GPU; every one that touches the library fails without the feature."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import build, capi, scene as S
from tests import rectifyref as R
from tests import temporalref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RADII = (1, 2, 3)
FLAGS = (0, R.REMODULATE, R.SHORTEN, R.REMODULATE | R.SHORTEN)
u32 = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


@pytest.fixture(scope="module")
def syn():
    return R.synthetic()


@pytest.fixture(scope="module")
def refs(syn):
    """rectify64 of the synthetic input with both flags, per radius (computed once, never changed)"""
    return {r: R.rectify64(*R.planes(syn), R.params(67, 45, radius=r)) for r in RADII}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# header <-> library <-> binding
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_layout(lib, tmp_path):
    for name in ("skh_rectify_check", "skh_rectify", "skh_get_rectify_info"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    for method in ("rectify_device", "rectify", "rectify_info"):
        assert callable(getattr(capi.Context, method))
    dt = S.RECTIFY_PARAMS
    fields = ("width", "height", "radius", "k", "albedo_floor", "flags", "reserved")
    assert dt.itemsize == 56 and dt.names == fields and [dt.fields[n][1] for n in fields] == [0, 4, 8, 12, 16, 20, 24]
    assert (S.RECTIFY_REMODULATE, S.RECTIFY_SHORTEN) == (1, 2) == (R.REMODULATE, R.SHORTEN)
    info = ("calls", "pixels", "ms_last")
    assert capi.RECTIFY_INFO.itemsize == 24 and capi.RECTIFY_INFO.names == info and [capi.RECTIFY_INFO.fields[n][1] for n in info] == [0, 8, 16]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu", sizeof(skh_rectify_params), sizeof(skh_rectify_info));\n'
                   + "".join(f'printf(" %zu", offsetof(skh_rectify_params, {f}));\n' for f in fields) + "".join(f'printf(" %zu", offsetof(skh_rectify_info, {f}));\n' for f in info)
                   + 'printf(" %u %u\\n", SKH_RECTIFY_REMODULATE, SKH_RECTIFY_SHORTEN); return SKH_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0 and lib.skh_abi_version() == 5  # the ABI grew, it did not change
    assert out.stdout.split() == [b"56", b"24", b"0", b"4", b"8", b"12", b"16", b"20", b"24", b"0", b"8", b"16", b"1", b"2"]
    assert "skh_rectify.h" in [os.path.basename(d) for d in build.DEPS]


def edited(**edits):
    p = S.rectify_params(67, 45)
    for n, v in edits.items():
        if n == "reserved":
            p["reserved"][v[0]] = v[1]
        else:
            p[n] = v
    return p


ACCEPTED = {"the defaults": edited(), "radius 1": edited(radius=1), "radius 2": edited(radius=2), "radius 3": edited(radius=3), "k = +inf": edited(k=np.inf),
            "a tiny k": edited(k=1e-30), "no flag": edited(flags=0), "both flags": edited(flags=3), "1 x 1": edited(width=1, height=1),
            "2^26 pixels": edited(width=1 << 13, height=1 << 13), "one row of 2^26": edited(width=1 << 26, height=1)}
REFUSED = {"width 0": edited(width=0), "height 0": edited(height=0), "2^26 + 2^13 pixels": edited(width=(1 << 13) + 1, height=1 << 13), "radius 0": edited(radius=0),
           "radius 4": edited(radius=4), "radius 2^32 - 1": edited(radius=0xFFFFFFFF), "k = 0": edited(k=0.0), "k < 0": edited(k=-2.0), "k = -inf": edited(k=-np.inf),
           "k NaN": edited(k=np.nan), "albedo_floor 0": edited(albedo_floor=0.0), "albedo_floor < 0": edited(albedo_floor=-0.05), "albedo_floor inf": edited(albedo_floor=np.inf),
           "albedo_floor NaN": edited(albedo_floor=np.nan), "flag bit 2": edited(flags=4), "flag bit 31": edited(flags=0x80000001), "reserved[0]": edited(reserved=(0, 1)),
           "reserved[7]": edited(reserved=(7, 9))}


def test_rectify_check_accepts_and_refuses(lib):
    for name, p in ACCEPTED.items():
        assert capi.rectify_check(p), name
    for name, p in REFUSED.items():
        assert not capi.rectify_check(p), name
        assert lib.skh_rectify_check(p.ctypes.data_as(C.c_void_p)) == 3, name
    # without parameters, a context or pointers the entry points refuse instead of crashing
    assert lib.skh_rectify_check(None) == 3 and lib.skh_rectify(None, None, None, None, None, None, None, None, None, None) == 3
    assert lib.skh_get_rectify_info(None, None) == 3


def test_rectify_params_defaults_and_round_trip():
    p = S.rectify_params(640, 360)
    assert (int(p["width"]), int(p["height"]), int(p["radius"]), float(p["k"])) == (640, 360, S.RECTIFY_RADIUS, S.RECTIFY_K)
    assert float(p["albedo_floor"]) == float(f32(S.DENOISE_ALBEDO_FLOOR)) and not p["reserved"].any()
    assert int(p["flags"]) == S.RECTIFY_REMODULATE | (S.RECTIFY_SHORTEN if S.RECTIFY_SHORTEN_DEFAULT else 0)
    assert S.RECTIFY_RADIUS in RADII and S.RECTIFY_K > 0 and 1.0 <= S.RECTIFY_FAST_HISTORY < S.TEMPORAL_MAX_HISTORY
    q = S.rectify_params(5, 7, radius=3, k=1.5, shorten=False, albedo_floor=0.25, remodulate=False)
    assert (int(q["width"]), int(q["height"]), int(q["radius"]), float(q["k"]), float(q["albedo_floor"]), int(q["flags"])) == (5, 7, 3, 1.5, 0.25, 0)
    assert int(S.rectify_params(5, 7, shorten=True, remodulate=False)["flags"]) == S.RECTIFY_SHORTEN
    back = np.frombuffer(q.tobytes(), S.RECTIFY_PARAMS)[0]
    assert back == q and q.tobytes()[:24] == np.array([5, 7, 3], np.uint32).tobytes() + np.array([1.5, 0.25], f32).tobytes() + np.array([0], np.uint32).tobytes()
    # the fast history's temporal record is one skh_temporal accepts
    t = S.temporal_params(5, 7, plane_tolerance=0.1, max_history=S.RECTIFY_FAST_HISTORY, initial_length=1.0)
    assert capi.temporal_check(t)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the synthetic input
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_synthetic_input_meets_its_conditions(syn, refs):
    ids, Hs, F = syn["ids"], syn["history"], syn["fast"]
    h, w = ids.shape[:2]
    assert (h, w) == (45, 67)
    kind = ids[..., 3]
    assert (kind == 0).any() and (kind == 3).any() and (kind == 1).any() and (kind == 2).any()
    for r in RADII:
        ref = refs[r]
        rect, clear, taps = ref["rectified"], ref["rectified"] & ~ref["ambiguous"], ref["taps"]
        assert rect.sum() > 2000 and not rect[(kind == 0) | (kind == 3)].any()
        for c in range(3):  # clamped from below, from above and left alone, in each channel, decided beyond the bar
            b, a = ref["below"][..., c] & clear, ref["above"][..., c] & clear
            assert b.sum() > 100 and a.sum() > 100 and (clear & ~ref["below"][..., c] & ~ref["above"][..., c]).sum() > 100, (r, c)
        full = (2 * r + 1) ** 2
        yy, xx = np.mgrid[0:h, 0:w]
        border = (yy < r) | (yy >= h - r) | (xx < r) | (xx >= w - r)
        assert (taps[rect & ~border] == full).any() and (taps[rect & border] < full).all() and (rect & border).sum() > 100  # windows cut by the border
        inner = rect & ~border & (taps < full)
        assert inner.sum() > 100  # ... and by an instance edge (or a skipped record)
        # the lone pixel: its only taken tap is itself, sd = 0, lo = hi = its own fast value
        assert rect[R.LONE] and taps[R.LONE] == 1
        assert np.array_equal(ref["lo"][R.LONE], F[R.LONE][:3].astype(np.float64)) and np.array_equal(ref["hi"][R.LONE], ref["lo"][R.LONE])
        # a NaN, an inf and a length below 1 in FAST: the centre is not rectified, and its neighbours of the same instance skip it
        for y, x in (R.FAST_NAN, R.FAST_INF, R.FAST_SHORT):
            assert not rect[y, x] and (kind[y, x] in (1, 2)) and R.record_mask(Hs)[y, x]
            nb = rect[y, x + 1] and ids[y, x + 1, 0] == ids[y, x, 0] and not border[y, x + 1]
            assert nb and taps[y, x + 1] < full
        # a record HISTORY does not have: not rectified either
        assert not rect[5, 5] and not rect[6, 60] and not rect[40, 33]
        # under a set mask, both nf < n (SHORTEN shortens) and nf >= n (it does not)
        set_ = clear & (ref["info"][..., 0] != 0)
        shorter = F[..., 3] < Hs[..., 3]
        assert (set_ & shorter).sum() > 100 and (set_ & ~shorter).sum() > 100
        assert np.array_equal(ref["history"][set_ & shorter][:, 3], F[set_ & shorter][:, 3]) and np.array_equal(ref["history"][set_ & ~shorter][:, 3], Hs[set_ & ~shorter][:, 3])
        unset = clear & (ref["info"][..., 0] == 0)
        assert (unset & shorter).sum() > 10 and np.array_equal(ref["history"][unset][:, 3], Hs[unset][:, 3])


def test_rectify64_alone_stays_within_the_ambiguity_cap(refs):
    for r in RADII:
        share = float(refs[r]["ambiguous"].sum()) / int(refs[r]["rectified"].sum())
        print(f"radius {r}: {int(refs[r]['ambiguous'].sum())} ambiguous of {int(refs[r]['rectified'].sum())} rectified pixels")
        assert share <= R.MAX_AMBIGUOUS_SHARE


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the float32 restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("flags", FLAGS)
def test_rectify32_within_rectify64s_bar(syn, radius, flags):
    p = R.params(67, 45, radius=radius, flags=flags)
    got, ref = R.rectify32(*R.planes(syn), p), R.rectify64(*R.planes(syn), p)
    worst, share = R.check(got, ref)
    print(f"radius {radius} flags {flags}: worst error / bar {worst:.3f}, ambiguous share {share:.5f}")
    assert worst <= 1.0
    if not flags & R.REMODULATE:  # the image is the history's rgb
        assert np.array_equal(u32(got["image"])[ref["rectified"]][:, :3], u32(got["history"])[ref["rectified"]][:, :3])
    unclamped = ref["rectified"] & (got["info"][..., 0] == 0)
    assert unclamped.sum() > 10 and np.array_equal(u32(got["history"])[unclamped], u32(syn["history"])[unclamped])
    if flags & R.REMODULATE:  # skh_temporal computed ill m in the same way: an unclamped pixel keeps the image's bits
        assert np.array_equal(u32(got["image"])[unclamped], u32(syn["image"])[unclamped])


@pytest.mark.parametrize("radius", RADII)
def test_infinite_k_returns_both_inputs(syn, radius):
    got = R.rectify32(*R.planes(syn), R.params(67, 45, radius=radius, k=np.inf))
    assert np.array_equal(u32(got["image"]), u32(syn["image"])) and np.array_equal(u32(got["history"]), u32(syn["history"]))
    rect = R.rectified_mask(syn["ids"], syn["history"], syn["fast"])
    assert not got["info"][..., 0].any() and not got["info"][..., 2].any() and np.array_equal(got["info"][rect][:, 3], syn["history"][rect][:, 3])


def test_a_constant_fast_plane_clamps_onto_the_constant(syn):
    fast = np.array(syn["fast"])
    fast[..., :3] = f32(0.375)
    for radius in RADII:
        got = R.rectify32(syn["image"], syn["ids"], syn["albedo"], syn["history"], fast, R.params(67, 45, radius=radius, flags=R.SHORTEN))
        rect = R.rectified_mask(syn["ids"], syn["history"], fast)
        assert rect.sum() > 2000 and (got["history"][rect][:, :3] == f32(0.375)).all() and (got["image"][rect][:, :3] == f32(0.375)).all()
        moved = (syn["history"][rect][:, :3] != f32(0.375)).astype(int) @ np.array([1, 2, 4])
        assert np.array_equal(got["info"][rect][:, 0], moved.astype(f32))


def test_unit_albedo_remodulation_is_no_remodulation(syn):
    ones = np.ones_like(syn["albedo"])
    a = R.rectify32(syn["image"], syn["ids"], ones, syn["history"], syn["fast"], R.params(67, 45, radius=2, flags=R.REMODULATE))
    b = R.rectify32(syn["image"], syn["ids"], None, syn["history"], syn["fast"], R.params(67, 45, radius=2, flags=0))
    for n in ("image", "history", "info"):
        assert np.array_equal(u32(a[n]), u32(b[n])), n


@pytest.mark.parametrize("radius", RADII)
def test_a_nan_in_fast_reaches_no_further_than_the_radius(syn, radius):
    p = R.params(67, 45, radius=radius)
    y, x = 17, 23
    assert R.rectified_mask(syn["ids"], syn["history"], syn["fast"])[y, x]
    fast = np.array(syn["fast"])
    fast[y, x, 0] = np.nan
    a, b = R.rectify32(*R.planes(syn), p), R.rectify32(syn["image"], syn["ids"], syn["albedo"], syn["history"], fast, p)
    differs = np.zeros((45, 67), bool)
    for n in ("image", "history", "info"):
        differs |= (u32(a[n]) != u32(b[n])).any(-1)
    yy, xx = np.mgrid[0:45, 0:67]
    near = (np.abs(yy - y) <= radius) & (np.abs(xx - x) <= radius)
    assert differs[y, x] and differs.sum() > 1 and not differs[~near].any()


def test_stepped_sequence_rectified_error_falls_below_unrectified():
    """A static image plus seeded noise through temporalref.reproject32 with the identity matrix: the level of a rectangle changes at frame 16.  Eight frames
    later the long history alone still holds 24 / 32 of the old level there; clamped to the fast history's window it must be nearer the new one.  Outside the
    rectangle rectification must not cost the accumulation: the error stays below a single frame's."""
    h, w = 24, 32
    rs = np.random.RandomState(11)
    ids = np.zeros((h, w, 4), np.uint32)
    ids[..., 3] = 1
    N, P, A = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32), np.ones((h, w, 4), f32)
    N[..., 2] = 1.0
    yy, xx = np.mgrid[0:h, 0:w]
    P[..., 0], P[..., 1] = (xx + 0.5) / w * 2 - 1, (yy + 0.5) / h * 2 - 1  # clip = P with the identity: every pixel projects onto itself
    P[..., 3] = N[..., 3] = 1.0
    rectangle = (yy >= 8) & (yy < 16) & (xx >= 10) & (xx < 22)
    tl = T.params(w, h, None, plane_tolerance=0.5, max_history=32.0)
    tf = T.params(w, h, None, plane_tolerance=0.5, max_history=float(S.RECTIFY_FAST_HISTORY))
    rp = S.rectify_params(w, h)
    long_plain = long_rect = fast = None
    for frame in range(24):
        level = np.where(rectangle, 0.2 if frame >= 16 else 0.8, 0.5)
        C = np.zeros((h, w, 4), f32)
        C[..., :3] = level[..., None] + rs.normal(0.0, 0.08, (h, w, 3))
        C[..., 3] = 1.0
        prev = lambda hist: None if hist is None else {"history": hist, "ids": ids, "normal": N, "position": P}
        long_plain = T.reproject32(C, ids, N, P, A, prev(long_plain), tl)["history"]
        t = T.reproject32(C, ids, N, P, A, prev(long_rect), tl)
        fast = T.reproject32(C, ids, N, P, A, prev(fast), tf)["history"]
        long_rect = R.rectify32(t["image"], ids, A, t["history"], fast, rp)["history"]
    rms = lambda a, m: float(np.sqrt(np.mean((a[..., :3][m].astype(np.float64) - level[m][:, None]) ** 2)))
    plain_in, rect_in, rect_out, raw_out = rms(long_plain, rectangle), rms(long_rect, rectangle), rms(long_rect, ~rectangle), rms(C, ~rectangle)
    print(f"in the rectangle, 8 frames after the step: rms {plain_in:.4f} unrectified, {rect_in:.4f} rectified; outside {rect_out:.4f} rectified, {raw_out:.4f} one frame")
    assert rect_in < plain_in and rect_out < raw_out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# oka::HipRender's parameter mapping
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_hiprender_parameter_mapping_from_a_standalone_program(lib, tmp_path):
    """tests/cpp/hiprender_rectify_main.cpp: integration/HipRender.h's HipRectify and hipRectifyParams with the C header and the library alone -- the defaults are
    scene.py's, a given field is taken as it is, and what comes out passes or fails skh_rectify_check as the same record does through the binding"""
    exe = str(tmp_path / "hiprender_rectify")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "hiprender_rectify_main.cpp"),
                           "-L" + libdir, "-lstrelka_hip", "-Wl,-rpath," + libdir])
    #        radius k fastHistory shorten width height albedoFloor
    cases = [(0, 0.0, 0.0, 1, 1920, 1080, 0.05),
             (3, 1.5, 8.0, 0, 67, 45, 0.1),
             (2, float("inf"), 1.0, 1, 1, 1, 0.05),
             (4, 2.0, 4.0, 1, 64, 64, 0.05),   # refused: the radius
             (1, -1.0, 4.0, 1, 64, 64, 0.05),  # refused: k
             (1, 2.0, 0.5, 1, 64, 64, 0.05),   # refused: the fast history's temporal record
             (1, 2.0, 4.0, 1, 0, 64, 0.05),    # refused: no image
             (1, 2.0, 4.0, 1, 64, 64, 0.0)]    # refused: the floor
    lines = ["%d %r %r %d %d %d %r" % c for c in cases]
    out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.decode().strip().split("\n")
    assert got[0].split() == ["56", "24"] and len(got) == 2 + len(cases)
    # a default-constructed HipRectify is scene.py's defaults
    cases = [(S.RECTIFY_RADIUS, S.RECTIFY_K, S.RECTIFY_FAST_HISTORY, int(S.RECTIFY_SHORTEN_DEFAULT), 1920, 1080, 0.05)] + cases
    for c, line in zip(cases, got[1:]):
        words = line.split()
        rec = np.frombuffer(np.array([int(w, 16) for w in words[:14]], np.uint32).tobytes(), S.RECTIFY_PARAMS)[0]
        fast = np.array([int(words[14], 16)], np.uint32).view(f32)[0]
        want = S.rectify_params(c[4], c[5], radius=c[0] or S.RECTIFY_RADIUS, k=c[1] or S.RECTIFY_K, shorten=bool(c[3]), albedo_floor=c[6])
        assert rec.tobytes() == want.tobytes(), (c, rec, want)
        assert fast == f32(c[2] or S.RECTIFY_FAST_HISTORY)
        assert int(words[15]) == (0 if capi.rectify_check(want) else 3)
    assert [(int(line.split()[15]), int(line.split()[16])) for line in got[1:]] == [(0, 0)] * 4 + [(3, 0), (3, 0), (0, 3), (3, 0), (3, 0)]
