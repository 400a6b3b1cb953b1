"""Temporal accumulation off the GPU ("Temporal accumulation"): the ABI's symbols and the records' layout through the C compiler;
skh_temporal_check's accept / refuse table; the conditions the synthetic input of tests/temporalref.py must meet; the float32 restatement of the definition
against the float64 reference's error bar; the definition's closed forms, bit for bit, on the float32 restatement; scene.temporal_params; and HipRender's
parameter mapping through a stand-alone program (tests/cpp/hiptemporal_params_main.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import build, capi, scene as S
from tests import temporalref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# header <-> library <-> binding
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_layout(lib, tmp_path):
    for name in ("skh_temporal_check", "skh_temporal", "skh_get_temporal_info"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    for method in ("temporal", "temporal_device", "temporal_info"):
        assert callable(getattr(capi.Context, method))
    dt = S.TEMPORAL_PARAMS
    fields = ("width", "height", "prev_world_to_clip", "normal_min", "plane_tolerance", "max_history", "initial_length", "albedo_floor", "flags", "reserved")
    assert dt.itemsize == 128 and dt.names == fields
    assert [dt.fields[n][1] for n in fields] == [0, 4, 8, 72, 76, 80, 84, 88, 92, 96]
    info = ("calls", "pixels", "ms_last")
    assert capi.TEMPORAL_INFO.itemsize == 24 and capi.TEMPORAL_INFO.names == info and [capi.TEMPORAL_INFO.fields[n][1] for n in info] == [0, 8, 16]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu", sizeof(skh_temporal_params), sizeof(skh_temporal_info));\n'
                   + "".join(f'printf(" %zu", offsetof(skh_temporal_params, {f}));\n' for f in fields) + "".join(f'printf(" %zu", offsetof(skh_temporal_info, {f}));\n' for f in info)
                   + 'printf(" %u\\n", SKH_TEMPORAL_DEMODULATE); return SKH_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0  # SKH_ABI_VERSION == 5: the ABI grew, it did not change
    assert out.stdout.split() == [b"128", b"24"] + [str(dt.fields[n][1]).encode() for n in fields] + [b"0", b"8", b"16", b"1"]
    assert S.TEMPORAL_DEMODULATE == 1 == R.DEMODULATE
    assert "skh_temporal.h" in [os.path.basename(d) for d in build.DEPS]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_temporal_check
# ---------------------------------------------------------------------------------------------------------------------------------------------
def good(**kw):
    args = dict(width=67, height=45, plane_tolerance=0.05)
    args.update(kw)
    return S.temporal_params(args.pop("width"), args.pop("height"), **args)


def edited(field, value, index=None, **kw):
    p = good(**kw)
    if index is None:
        p[field] = value
    else:
        p[field][index] = value
    return p


ACCEPTED = {"the defaults": good(), "one pixel": good(width=1, height=1), "2^26 pixels": good(width=1 << 13, height=1 << 13), "2^26 in a row": good(width=1 << 26, height=1),
            "no flag": good(demodulate=False), "normal_min -1": good(normal_min=-1.0), "normal_min 1": good(normal_min=1.0), "plane_tolerance +inf": good(plane_tolerance=INF),
            "a tiny tolerance": good(plane_tolerance=1e-30), "max_history 1": good(max_history=1.0), "initial_length == max_history": good(initial_length=32.0),
            "a fractional length": good(initial_length=2.5), "a tiny floor": good(albedo_floor=1e-30), "a huge matrix entry": edited("prev_world_to_clip", 3e38, 7)}
REFUSED = {"zero width": good(width=0), "zero height": good(height=0), "2^26 + 2^13 pixels": good(width=(1 << 13) + 1, height=1 << 13),
           "a product that wraps 32 bits": good(width=1 << 16, height=1 << 16), "matrix nan": edited("prev_world_to_clip", np.nan, 0), "matrix inf": edited("prev_world_to_clip", INF, 15),
           "matrix -inf": edited("prev_world_to_clip", -INF, 9), "normal_min 1.0001": good(normal_min=1.0001), "normal_min -1.0001": good(normal_min=-1.0001),
           "normal_min nan": good(normal_min=np.nan), "normal_min inf": good(normal_min=INF), "plane_tolerance 0": good(plane_tolerance=0.0), "plane_tolerance -0": good(plane_tolerance=-0.0),
           "plane_tolerance < 0": good(plane_tolerance=-1.0), "plane_tolerance nan": good(plane_tolerance=np.nan), "plane_tolerance -inf": good(plane_tolerance=-INF),
           "max_history 0.999": good(max_history=0.999), "max_history 0": good(max_history=0.0), "max_history inf": good(max_history=INF), "max_history nan": good(max_history=np.nan),
           "initial_length 0.999": good(initial_length=0.999), "initial_length 0": good(initial_length=0.0), "initial_length above max_history": good(initial_length=32.5),
           "initial_length inf": good(initial_length=INF, max_history=32.0), "initial_length nan": good(initial_length=np.nan),
           "floor 0": good(albedo_floor=0.0), "floor < 0": good(albedo_floor=-0.1), "floor inf": good(albedo_floor=INF), "floor nan": good(albedo_floor=np.nan),
           "flag bit 1": edited("flags", 2), "flag bit 31": edited("flags", 0x80000001), "reserved[0]": edited("reserved", 1, 0), "reserved[7]": edited("reserved", 9, 7)}


def test_temporal_check_accepts_and_refuses(lib):
    for name, p in ACCEPTED.items():
        assert capi.temporal_check(p), name
    for name, p in REFUSED.items():
        assert not capi.temporal_check(p), name
        assert lib.skh_temporal_check(p.ctypes.data_as(C.c_void_p)) == 3, name
    assert lib.skh_temporal_check(None) == 3
    # without a context the entry points refuse instead of crashing
    assert lib.skh_temporal(*([None] * 14)) == 3 and lib.skh_get_temporal_info(None, None) == 3


def test_temporal_params_defaults_and_round_trip():
    from strelka_amd import scenes

    sc = scenes.cornell_box()
    arr = sc.arrays()
    aov = S.aov_params(sc.getCamera(), 96, 64)
    p = S.temporal_params(96, 64, aov, scene=arr)
    assert (int(p["width"]), int(p["height"]), int(p["flags"])) == (96, 64, S.TEMPORAL_DEMODULATE) and not p["reserved"].any()
    assert np.array_equal(p["prev_world_to_clip"], aov["world_to_clip"])
    assert [float(p[k]) for k in ("normal_min", "max_history", "initial_length", "albedo_floor")] == [f32(0.9), 32.0, 1.0, f32(S.DENOISE_ALBEDO_FLOOR)]
    assert float(p["plane_tolerance"]) == f32(S.DENOISE_PLANE_FRACTION * S.scene_diagonal(arr)) and capi.temporal_check(p)
    q = S.temporal_params(8, 4, normal_min=0.5, plane_tolerance=0.125, max_history=8.0, initial_length=3.0, albedo_floor=0.0625, demodulate=False)
    assert [float(q[k]) for k in ("normal_min", "plane_tolerance", "max_history", "initial_length", "albedo_floor")] == [0.5, 0.125, 8.0, 3.0, 0.0625] and int(q["flags"]) == 0
    assert np.array_equal(q["prev_world_to_clip"].reshape(4, 4), np.eye(4, dtype=f32))  # (no previous frame: a matrix the check accepts)
    r = np.frombuffer(q.tobytes(), S.TEMPORAL_PARAMS)[0]
    assert r.tobytes() == q.tobytes() and capi.temporal_check(r)
    with pytest.raises(ValueError):
        S.temporal_params(8, 8)  # plane_tolerance is in scene units: no scene, no default


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the synthetic input, and float32 against float64
# ---------------------------------------------------------------------------------------------------------------------------------------------
def both(s, p=None, prev=True):
    a = (s["color"], s["ids"], s["normal"], s["position"], s["albedo"], s["prev"] if prev else None, s["params"] if p is None else p)
    return R.reproject32(*a), R.reproject64(*a)


def test_the_synthetic_input_meets_its_conditions():
    s = R.synthetic()
    assert s["ids"].shape == (45, 67, 4)
    got, ref = both(s)
    surf, n = ref["surface"], int(ref["surface"].sum())
    kind, pkind = s["ids"][..., 3], s["prev"]["ids"][..., 3]
    # what is planted: a NaN pixel, a miss region and a light-proxy kind in each frame; history lengths that are mixed and include 0
    assert (kind == 0).sum() >= 24 and (kind == 3).sum() == 24 and (pkind == 0).sum() >= 21 and (pkind == 3).sum() == 18 and (kind == 2).any() and (pkind == 2).any()
    assert np.isnan(s["color"][..., :3]).sum() == 1 and np.isinf(s["color"][..., :3]).sum() == 1 and np.isnan(s["prev"]["history"]).sum() == 2
    lengths = s["prev"]["history"][..., 3][(pkind == 1) | (pkind == 2)]
    assert set(np.unique(lengths[np.isfinite(lengths)])) == {0.0, 1.0, 2.0, 5.0, 8.0, 17.5, 32.0}
    # no surface pixel is excluded for any reason other than ambiguity, and those are few
    assert n == int((((kind == 1) | (kind == 2)) & np.isfinite(s["color"][..., :3]).all(-1)).sum()) and n > 0.8 * kind.size
    share = ref["ambiguous"].sum() / n
    acc = ref["accepted"][surf]
    none, some, four = (acc == 0).mean(), ((acc > 0) & (acc < 4)).mean(), (acc == 4).mean()
    print(f"synthetic 67 x 45: {n} surface pixels of {kind.size}, ambiguous {int(ref['ambiguous'].sum())} ({100 * share:.3f} %); accepted taps: none {none:.3f}, "
          f"one to three {some:.3f}, four {four:.3f}; pixels that do not project {1 - ref['projects'][surf].mean():.3f}")
    assert share <= 0.02 and none >= 0.05 and some >= 0.05 and four >= 0.5
    # every kind of rejection happens: outside the previous image, another instance, a dropped or non-finite history, the normal, the plane
    assert (~ref["projects"] & surf).sum() > 50
    loose = np.array(s["params"])
    loose["normal_min"], loose["plane_tolerance"] = -1.0, INF
    _, ref_loose = both(s, loose)
    assert (ref_loose["accepted"] > ref["accepted"]).sum() > 20  # (the two geometric tests reject taps the exact tests pass)


@pytest.mark.parametrize("prev", [True, False])
@pytest.mark.parametrize("flags", [R.DEMODULATE, 0])
def test_float32_evaluation_stays_inside_the_bar(flags, prev):
    s = R.synthetic()
    p = np.array(s["params"])
    p["flags"] = flags
    got, ref = both(s, p, prev)
    ratio = R.check(got, s["color"], ref)
    widest = {n: float(ref["bar_" + n].max()) for n in ("image", "history", "motion")}
    print(f"flags {flags}, {'a' if prev else 'no'} previous frame: float32 evaluation, worst error / bar {ratio:.3f}; widest bars {widest}")
    assert ratio <= 1.0
    if prev:
        # the bars are not orders of magnitude too wide: a fraction of a thousandth of a pixel for the motion, 1e-3 of a colour of order 1
        assert ratio > 0.005 and ref["bar_motion"][..., :2].max() < 1e-4 and np.median(ref["bar_image"][ref["accepted"] > 0]) < 1e-5


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (64, 64), (65, 63)])
def test_the_shapes_of_the_device_test_are_well_formed(w, h):
    s = R.synthetic(w, h, seed=w + h)
    got, ref = both(s)
    assert R.check(got, s["color"], ref) <= 1.0 and ref["surface"].any()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# closed forms, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def planar(n, shift=(0.0, 0.0), seed=11):
    """an n x n image (n a power of two) of the plane z = 0, P = (px + 0.5, py + 0.5, 0), N = +z, one instance, unit albedo, and the matrix that maps P to the pixel
    it came from moved by `shift`: clip.x = (2 / n) (P.x + shift.x) - 1, clip.w = 1 -- powers of two throughout, so that fx = px + shift.x exactly"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    ids = np.zeros((n, n, 4), np.uint32)
    ids[..., 3] = 1
    N, P, A = np.zeros((n, n, 4), np.float32), np.zeros((n, n, 4), np.float32), np.ones((n, n, 4), np.float32)
    N[..., 2], P[..., 0], P[..., 1], P[..., 3] = 1.0, x + 0.5, y + 0.5, 1.0
    M = np.zeros((4, 4), np.float32)
    M[0, 0] = M[1, 1] = 2.0 / n
    M[0, 3], M[1, 3] = 2.0 * shift[0] / n - 1.0, 2.0 * shift[1] / n - 1.0
    M[2, 2] = M[3, 3] = 1.0
    C = np.ones((n, n, 4), np.float32)
    C[..., :3] = rs.uniform(0.0, 2.0, (n, n, 3))
    Hs = np.zeros((n, n, 4), np.float32)
    Hs[..., :3], Hs[..., 3] = rs.uniform(0.0, 2.0, (n, n, 3)), 1.0
    return {"color": C, "ids": ids, "normal": N, "position": P, "albedo": A, "prev": {"history": Hs, "ids": ids.copy(), "normal": N.copy(), "position": P.copy()},
            "params": R.params(n, n, M, plane_tolerance=0.5, flags=0)}


def run32(s, p=None, **planes):
    """reproject32 on the input `s`, with `planes` in place of its own"""
    t = dict(s, **planes)
    return R.reproject32(t["color"], t["ids"], t["normal"], t["position"], t["albedo"], t["prev"], s["params"] if p is None else p)


def test_an_integer_shift_fetches_the_shifted_history_and_half_a_pixel_averages_two_taps():
    n = 32
    for k in (0, 3, -5):
        s = planar(n, shift=(k, 0))
        got = run32(s)
        x = np.arange(n)
        inside, projects = (x + k >= 0) & (x + k < n), (x + k >= -1) & (x + k <= n)
        assert np.array_equal(got["motion"][..., 0], np.tile(np.where(projects, k, 0).astype(f32), (n, 1))) and not got["motion"][..., 1].any()  # fx = px + k exactly
        hist, c = s["prev"]["history"], s["color"][..., :3]
        h = hist[:, np.clip(x + k, 0, n - 1), :3]
        want = h + (c - h) * f32(0.5)  # n = 1 -> n' = 2, alpha = 1/2
        assert np.array_equal(bits(got["history"][:, inside, :3]), bits(want[:, inside])) and (got["history"][:, inside, 3] == 2.0).all()
        assert (got["motion"][:, inside, 2] == 1.0).all() and (got["motion"][:, inside, 3] == 1.0).all()  # the whole weight on tap 0, the only one with a weight > 0
        # ... and where the shift leaves the image there is no history (fx = -1 or n still projects, its taps lie outside or weigh 0; beyond that nothing projects)
        assert np.array_equal(bits(got["history"][:, ~inside, :3]), bits(c[:, ~inside])) and (got["history"][:, ~inside, 3] == 1.0).all()
    s = planar(n, shift=(0.5, 0))
    got = run32(s)
    hist, c = s["prev"]["history"], s["color"][..., :3]
    h = (f32(0.5) * hist[:, :-1, :3] + f32(0.5) * hist[:, 1:, :3]) / f32(1.0)
    assert np.array_equal(bits(got["history"][:, :-1, :3]), bits(h + (c[:, :-1] - h) * f32(0.5))) and (got["motion"][:, :-1, 3] == 3.0).all()
    assert (got["motion"][:, -1, 3] == 1.0).all() and np.array_equal(bits(got["history"][:, -1, :3]), bits(hist[:, -1, :3] + (c[:, -1] - hist[:, -1, :3]) * f32(0.5)))


def test_feeding_frames_back_gives_the_running_mean_and_max_history_holds_alpha():
    n, K = 16, 12
    s = planar(n)
    rs = np.random.RandomState(2)
    frames = [np.concatenate([rs.uniform(0.0, 2.0, (n, n, 3)), np.ones((n, n, 1))], -1).astype(f32) for _ in range(K)]
    for cap in (32.0, 4.0):
        p = np.array(s["params"])
        p["max_history"] = cap
        hist, mean = None, np.zeros((n, n, 3))
        for k, frame in enumerate(frames):
            prev = None if hist is None else dict(s["prev"], history=hist)
            got = R.reproject32(frame, s["ids"], s["normal"], s["position"], s["albedo"], prev, p)
            hist = got["history"]
            assert np.array_equal(bits(got["image"]), bits(np.concatenate([hist[..., :3], frame[..., 3:]], -1)))  # (no DEMODULATE: the image is the illumination)
            if cap >= K:
                # the arithmetic mean of the k + 1 inputs.  Roundings: step j (j >= 2) computes h + (c - h) / j -- the difference, the quotient 1 / j, the product
                # and the sum, 4 u of values below 2 each -- and passes the earlier error on with the factor (1 - 1/j) <= 1: at most 4 (k + 1) u 2 after k + 1 frames
                mean += (frame[..., :3].astype(np.float64) - mean) / (k + 1)
                assert (hist[..., 3] == k + 1).all() and np.abs(hist[..., :3] - mean).max() <= 4 * (k + 1) * R.U * 2.0
            else:
                assert (hist[..., 3] == min(k + 1, cap)).all()  # alpha = 1/4 from the fourth frame on
                if k >= 4:
                    assert np.array_equal(bits(hist[..., :3]), bits(before + (frame[..., :3] - before) * f32(0.25)))
            before = hist[..., :3].copy()


def test_constants_stay_constant():
    def constant(shift):
        s = planar(16, shift=shift)
        s["color"][..., :3], s["prev"]["history"][..., :3] = [0.3, 1.7, 1e-3], [0.3, 1.7, 1e-3]
        s["prev"]["history"][..., 3] = 5.0
        return s, run32(s)

    # half a pixel in x: two taps of weight 1/2 (one at the border), every product, sum and quotient exact -- the bits stay
    s, got = constant((0.5, 0.0))
    assert (got["motion"][:, :-1, 3] == 3.0).all() and (got["motion"][:, -1, 3] == 1.0).all()
    assert np.array_equal(bits(got["image"]), bits(s["color"])) and np.array_equal(bits(got["history"][..., :3]), bits(s["color"][..., :3])) and (got["history"][..., 3] == 6.0).all()
    # weights in sixteenths: w v rounds, so the value comes back within the blend's count of roundings (9 u |v|, temporalref.py), and c - h then adds less than that
    s, got = constant((0.25, 0.75))
    assert (got["motion"][:-1, :-1, 3] == 15.0).all() and (got["history"][..., 3] == 6.0).all()
    assert (np.abs(got["image"][..., :3].astype(np.float64) - s["color"][..., :3]) <= 2 * 9 * R.U * s["color"][..., :3]).all()


def test_a_nan_in_one_previous_pixel_changes_only_the_pixels_that_tap_it():
    s = planar(16, shift=(0.5, 0.5))
    clean = run32(s)
    for word in range(4):
        hist = s["prev"]["history"].copy()
        hist[6, 9, word] = np.nan
        got = run32(s, prev=dict(s["prev"], history=hist))
        changed = (bits(got["history"]) != bits(clean["history"])).any(-1)
        ys, xs = np.nonzero(changed)
        assert set(zip(ys, xs)) == {(5, 8), (5, 9), (6, 8), (6, 9)}  # the four pixels whose 2 x 2 footprint holds (6, 9)
        assert np.isfinite(got["history"]).all() and np.isfinite(got["image"]).all()
        assert (got["motion"][changed][:, 3] == [7.0, 11.0, 13.0, 14.0]).all() and (got["motion"][changed][:, 2] == 0.75).all()  # the other three taps
    # all four taps of a pixel bad: no history, not a poisoned one
    hist = s["prev"]["history"].copy()
    hist[6:8, 9:11, 3] = 0.0
    got = run32(s, prev=dict(s["prev"], history=hist))
    assert got["motion"][6, 9, 3] == 0.0 and got["history"][6, 9, 3] == 1.0 and np.array_equal(bits(got["history"][6, 9, :3]), bits(s["color"][6, 9, :3]))
    assert got["motion"][6, 9, 0] == 0.5 and got["motion"][6, 9, 2] == 0.0  # (it projects: its motion is written, with sw = 0)


def test_pass_through_of_what_is_no_surface_pixel():
    s = R.synthetic()
    for flags in (0, 1):
        p = np.array(s["params"])
        p["flags"] = flags
        got = run32(s, p)
        kind = s["ids"][..., 3]
        other = (kind == 0) | (kind == 3) | ~np.isfinite(s["color"][..., :3]).all(-1)
        assert other.sum() > 40 + 2
        assert np.array_equal(bits(got["image"])[other], bits(s["color"])[other])
        assert np.array_equal(bits(got["image"])[..., 3], bits(s["color"])[..., 3])  # every alpha word, the NaN patterns among them
        assert not bits(got["history"])[other].any() and not bits(got["motion"])[other].any()
        assert np.array_equal(~np.isfinite(got["image"][..., :3]), ~np.isfinite(s["color"][..., :3]))  # nothing spread
        assert np.isfinite(got["history"]).all() and np.isfinite(got["motion"]).all()


def test_demodulation_with_unit_albedo_is_the_call_without_the_flag():
    s = R.synthetic()
    one = np.ones_like(s["albedo"])
    p0, p1 = np.array(s["params"]), np.array(s["params"])
    p0["flags"], p1["flags"] = 0, 1
    a, b = run32(s, p0, albedo=one), run32(s, p1, albedo=one)
    for n in ("image", "history", "motion"):
        assert np.array_equal(bits(a[n]), bits(b[n]))
    assert not np.array_equal(bits(run32(s, p1)["image"]), bits(a["image"]))  # (with the real albedo it is another picture)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# oka::HipRender's parameter mapping
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_hiprender_parameter_mapping_from_a_standalone_program(lib, tmp_path):
    """tests/cpp/hiptemporal_params_main.cpp: integration/HipRender.h's hipTemporalParams with the C header and the library alone -- the defaults are scene.py's, a
    given field is taken as it is, and what comes out passes or fails skh_temporal_check as the same record does through the binding"""
    exe = str(tmp_path / "hiptemporal_params")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "hiptemporal_params_main.cpp"),
                           "-L" + libdir, "-lstrelka_hip", "-Wl,-rpath," + libdir])
    #        normalMin planeTolerance planeFraction maxHistory albedoFloor width height initialLength sceneDiagonal withMatrix
    cases = [(0.0, 0.0, 0.0, 0.0, 0.0, 1920, 1080, 0.0, 12.5, 1),
             (0.5, 0.02, 0.5, 8.0, 0.1, 67, 45, 3.0, 12.5, 0),
             (-1.0, 0.0, 0.01, 0.0, 0.0, 1, 1, 32.0, 3.0, 1),
             (0.0, -1.0, -1.0, -1.0, -1.0, 640, 360, 1.0, 100.0, 0),
             (0.0, 0.0, 0.0, 0.0, 0.0, 64, 64, 0.0, 0.0, 1),  # nothing to measure: the plane test is off
             (1.5, 0.0, 0.0, 0.0, 0.0, 64, 64, 0.0, 1.0, 0),  # refused by the check
             (0.0, 0.0, 0.0, 4.0, 0.0, 64, 64, 5.0, 1.0, 0),  # a length above max_history
             (0.0, 0.0, 0.0, 0.0, 0.0, 0, 64, 0.0, 1.0, 1)]
    lines = ["%r %r %r %r %r %d %d %r %r %d" % c for c in cases]
    out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.decode().strip().split("\n")
    assert got[0].split() == ["128", "24"] and len(got) == 1 + len(cases)
    matrix = np.arange(1, 17, dtype=f32)
    for c, line in zip(cases, got[1:]):
        words = line.split()
        rec = np.frombuffer(np.array([int(w, 16) for w in words[:32]], np.uint32).tobytes(), S.TEMPORAL_PARAMS)[0]
        plane = f32(c[1]) if c[1] > 0 else f32(f32(c[2]) if c[2] > 0 else f32(S.DENOISE_PLANE_FRACTION)) * f32(c[8])
        want = S.temporal_params(c[5], c[6], {"world_to_clip": matrix} if c[9] else None, normal_min=c[0] if c[0] != 0 else S.TEMPORAL_NORMAL_MIN,
                                 plane_tolerance=plane if plane > 0 else INF, max_history=c[3] if c[3] > 0 else S.TEMPORAL_MAX_HISTORY,
                                 initial_length=c[7] if c[7] > 0 else 1.0, albedo_floor=c[4] if c[4] > 0 else S.DENOISE_ALBEDO_FLOOR)
        assert rec.tobytes() == want.tobytes(), (c, rec, want)
        assert int(words[32]) == (0 if capi.temporal_check(want) else 3)
    assert [int(line.split()[32]) for line in got[1:]] == [0, 0, 0, 0, 0, 3, 3, 3]
