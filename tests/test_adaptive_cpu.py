"""Adaptive sampling off the GPU ("Adaptive sampling"): the float32 restatement in tests/adaptref.py against its float64 twin within a
written-out count of roundings; properties of the schedule; parameter validation through the library (it loads without a GPU); header, binding and export list;
and the non-vacuity of the scene tests/test_gpu_adaptive.py renders, checked here with the CPU oracle (whose images equal the device's bit for bit)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import adaptref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24  # unit roundoff of float32

# The scene of the GPU tests: the Cornell box from far enough back that the border tiles see only void; 72 x 40 pixels, tile_size 8 (9 x 5 whole tiles).  The same
# image with tile_size 16 (PARTIAL_TILE) has tiles cut by both edges (72 = 4.5 x 16, 40 = 2.5 x 16): the second configuration of the schedule and image tests.
W, H, TILE, DEPTH, SPP, MIN_SAMPLES, INTERVAL = 72, 40, 8, 3, 32, 4, 4
PARTIAL_TILE = 16
EXPOSURE = np.full(3, 1.0, F)
CAMERA_Z = 7.0
# Chosen on the CPU oracle (test_the_gpu_scene_has_all_three_kinds_of_tile), before any device run: with these the reference schedule has tiles that freeze at the
# first check (the void), tiles that freeze at a later check, and tiles that run to SPP.  RECORDED_HIST: observations -> number of tiles, per tile size.
THRESHOLD, DARK_LEVEL = 0.1, 0.2
RECORDED_HIST = {8: {4: 36, 8: 3, 12: 1, 16: 1, 20: 1, 28: 2, 32: 1}, 16: {4: 11, 8: 1, 12: 1, 28: 1, 32: 1}}


def adaptive_scene():
    sc = scenes.cornell_box()
    sc.getCamera().lookAt((0.0, 0.0, CAMERA_Z), (0.0, 0.0, 0.0))
    return sc


def params(sc, i, spl=1, spp=SPP, **kw):
    return S.frame_params(sc.getCamera(), W, H, subframe_index=i, samples_this_launch=spl, spp_total=spp, max_depth=DEPTH, exposure=EXPOSURE, **kw)


def oracle_observations(sc, arr=None, launches=SPP, spl=1):
    """per-launch images of the CPU oracle with accumulation off: (launches, H, W, 3)"""
    from tests import orklib

    o = orklib.new_context()
    o.set_scene(sc.arrays() if arr is None else arr)
    o.resize(W, H)
    out = []
    for k in range(launches):
        o.render_subframe(params(sc, k * spl, spl, enable_accumulation=0))
        out.append(o.read_image()[..., :3].copy())
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float32 against float64
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ymax", [1.0, 1e-3])
def test_float32_restatement_within_its_roundings_of_float64(ymax):
    """n <= 64 observations y in [1e-6 ymax, ymax], log-uniform, plus constant and two-valued series.  The bars, first order in u = 2^-24, from the text of the update:
      mean: a step rounds d = y - mean (|d| <= ymax), d / n (<= ymax) and the sum (<= ymax): 3 roundings of at most u ymax each; the error already in mean enters the
            new mean with the factor (1 - 1/n) <= 1.  After n steps: E_mean <= 3 n u ymax; the bar takes 4 n u ymax for the second-order terms.
      M2:   a step multiplies d (error <= u ymax + E_mean) by y - mean' (the same), both <= ymax in size, rounds the product (u ymax^2) and the sum (u M2 <= u n ymax^2):
            <= ymax^2 u (2 (4 n + 1) + 1 + n) = ymax^2 u (9 n + 3) per step, n (9 n + 3) u ymax^2 after n steps.
      q:    M2 / n / n / (ref ref) with ref = max(mean, dark): relative error <= E_M2 / M2 + 2 E_mean / ref + 4 u (two divisions, the product, the last division)."""
    rs = np.random.RandomState(5)
    n = 64
    series = [np.exp(rs.uniform(np.log(1e-6), 0.0, (n, 256))) * ymax, np.full((n, 4), 0.37 * ymax), np.where(rs.rand(n, 64) < 0.1, ymax, 1e-6 * ymax)]
    ys = np.concatenate(series, 1).astype(F)
    dark = 0.05 * ymax
    for k in (2, 3, 17, 64):
        n32, m32, s32 = adaptref.welford(ys[:k], F)
        n64, m64, s64 = adaptref.welford(ys[:k], np.float64)
        assert m32.dtype == F and s32.dtype == F and m64.dtype == np.float64
        assert np.array_equal(n32, n64) and (n32 == k).all()
        e_mean, e_m2 = 4 * k * U * ymax, k * (9 * k + 3) * U * ymax * ymax
        assert np.abs(m32 - m64).max() <= e_mean
        assert np.abs(s32 - s64).max() <= e_m2
        q32, q64 = adaptref.pixel_q(n32, m32, s32, dark), adaptref.pixel_q(n64, m64, s64, dark)
        ref = np.maximum(m64, dark)
        bar = (e_m2 / (k * k * ref * ref)) + q64 * (2 * e_mean / ref + 4 * U) * 1.01
        assert (np.abs(q32 - q64) <= bar).all()
    # a constant series has no spread at all, in either precision
    assert (adaptref.welford(ys[:, 256:260], F)[2] == 0).all()


def test_luma_is_the_stated_formula():
    obs, e = np.array([[0.5, 2.0, 17.0]], F), np.array([0.25, 1.0, 2.0], F)
    c = obs[0] * e
    t = c / (c + F(1))
    want = F(F(F(0.2126) * t[0]) + F(F(0.7152) * t[1])) + F(F(0.0722) * t[2])
    got = adaptref.luma(obs, e)
    assert got.dtype == F and got[0] == F(want)
    assert adaptref.luma(obs, e, np.float64).dtype == np.float64


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------------------------------------------------
def noise_stack(seed=2, launches=32, h=20, w=28):
    rs = np.random.RandomState(seed)
    level = np.linspace(0.02, 3.0, w)[None, :, None] * np.ones((h, 1, 3))
    spread = np.linspace(0.0, 1.0, h)[:, None, None]
    return (level[None] * (1.0 + spread[None] * rs.uniform(-1, 1, (launches, h, w, 1)))).astype(F)


def test_freezing_is_monotone_in_the_threshold():
    obs, e = noise_stack(), np.ones(3, F)
    prev = None
    for thr in (0.0, 0.01, 0.03, 0.1, 0.3, 1.0):
        c = np.array(adaptref.schedule(obs, e, 8, thr, 0.05, 4, 4)["counts"])
        assert ((c >= 4) & (c <= 32) & (c % 4 == 0)).all()
        if prev is not None:
            assert (c <= prev).all(), thr  # a larger threshold never keeps a tile running longer
        prev = c
    assert (prev == 4).all()  # threshold 1: every tile of this stack stops at the first check
    c0 = np.array(adaptref.schedule(obs, e, 8, 0.0, 0.05, 4, 4)["counts"])
    assert (c0 == 32).all()  # threshold 0 stops only what has no spread at all: every tile of this stack has rows with some ...
    flat = np.array(adaptref.schedule(obs[:1].repeat(32, 0), e, 8, 0.0, 0.05, 4, 4)["counts"])
    assert (flat == 4).all()  # ... and the same image 32 times over has none


def test_min_samples_at_spp_total_freezes_nothing_before_the_end():
    obs, e = noise_stack(), np.ones(3, F)
    r = adaptref.schedule(obs, e, 8, 1.0, 0.05, 32, 4)
    assert (np.array(r["counts"]) == 32).all() and r["checks"] == 1
    r = adaptref.schedule(obs[:31], e, 8, 1.0, 0.05, 32, 4)
    assert (np.array(r["counts"]) == 31).all() and r["checks"] == 0 and (r["state"][..., 3] == 0).all()


def test_a_nan_never_freezes_and_partial_tiles_are_counted():
    obs, e = noise_stack(h=20, w=28), np.ones(3, F)
    obs = obs * 0 + F(0.5)  # no spread: everything stops at the first check ...
    obs[2, 3, 9, 1] = np.nan  # ... but the tile of pixel (9, 3)
    r = adaptref.schedule(obs, e, 8, 0.5, 0.05, 4, 4)
    cm = adaptref.count_map(r, 28, 20, 8)
    assert len(r["counts"]) == 4 * 3 and cm[3, 9] == 32 and (cm[:, 16:] == 4).all() and (cm[8:, :] == 4).all()
    assert r["state"][19, 27, 0] == 4 and r["state"][0, 8, 0] == 32


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the library: validation, symbols, records
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from strelka_amd import build, capi

    build.build()
    return capi.load()


def test_parameter_validation(lib):
    from strelka_amd import capi

    def check(*a):
        return lib.skh_adaptive_check(capi.adaptive_record(*a).ctypes.data_as(C.c_void_p))

    assert check(0.05, 0.01, 16, 8) == 0 and check(0.0, 1e-6, 2, 1) == 0
    for bad in ((-0.01, 0.01, 16, 8), (np.nan, 0.01, 16, 8), (np.inf, 0.01, 16, 8), (0.05, 0.0, 16, 8), (0.05, -1.0, 16, 8), (0.05, np.nan, 16, 8),
                (0.05, np.inf, 16, 8), (0.05, 0.01, 1, 8), (0.05, 0.01, 0, 8), (0.05, 0.01, 16, 0)):
        assert check(*bad) == 3, bad  # SKH_INVALID_ARGUMENT
    a = capi.adaptive_record(0.05, 0.01, 16, 8)
    a["reserved"][2] = 1
    assert lib.skh_adaptive_check(a.ctypes.data_as(C.c_void_p)) == 3
    assert lib.skh_adaptive_check(None) == 3
    # without a context every entry point refuses instead of crashing
    assert lib.skh_set_adaptive(None, None) == 3 and lib.skh_get_adaptive_info(None, None) == 3 and lib.skh_read_adaptive(None, None) == 3


def test_header_binding_and_export_list_agree(lib, tmp_path):
    from strelka_amd import capi

    header = open(os.path.join(ROOT, "include", "strelka_hip.h")).read()
    assert "#define SKH_INVALID_ARGUMENT" in header or re.search(r"SKH_INVALID_ARGUMENT\s*=\s*3", header)
    for name in ("skh_adaptive_check", "skh_set_adaptive", "skh_get_adaptive_info", "skh_read_adaptive"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in capi.SYMBOLS and hasattr(lib, name)
    assert int(re.search(r"#define SKH_ABI_VERSION (\d+)", header).group(1)) == 5  # additive
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(skh_adaptive), offsetof(skh_adaptive, threshold), offsetof(skh_adaptive, dark_level), offsetof(skh_adaptive, min_samples), "
                   "offsetof(skh_adaptive, interval), offsetof(skh_adaptive, reserved), sizeof(skh_adaptive_info), offsetof(skh_adaptive_info, active_tiles), "
                   "offsetof(skh_adaptive_info, max_observations), offsetof(skh_adaptive_info, pixel_observations), "
                   "offsetof(skh_adaptive_info, pixel_observations_saved)); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0 and [int(v) for v in out.stdout.split()] == [32, 0, 4, 8, 12, 16, 40, 8, 20, 24, 32]
    assert capi.ADAPTIVE.itemsize == 32 and [capi.ADAPTIVE.fields[n][1] for n in capi.ADAPTIVE.names] == [0, 4, 8, 12, 16]
    assert capi.ADAPTIVE_INFO.itemsize == 40 and [capi.ADAPTIVE_INFO.fields[n][1] for n in capi.ADAPTIVE_INFO.names] == [0, 4, 8, 12, 16, 20, 24, 32]


def test_dark_level_helper():
    from strelka_amd import capi

    e = np.array([0.5, 0.5, 0.5], F)
    want = adaptref.luma(np.full((1, 3), 0.1, F), e)[0]
    assert capi.adaptive_dark_level(0.1, e) == float(want) and 0 < want < 0.05


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the GPU tests' scene is not vacuous
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [TILE, PARTIAL_TILE])
def test_the_gpu_scene_has_all_three_kinds_of_tile(tile):
    """THRESHOLD 0.1, DARK_LEVEL 0.2 on the 72 x 40 Cornell box from z = 7, depth 3, 32 spp, checks at 4, 8, ..., 32: recorded on the CPU oracle"""
    sc = adaptive_scene()
    obs = oracle_observations(sc)
    assert obs.shape == (SPP, H, W, 3) and np.isfinite(obs).all()
    r = adaptref.schedule(obs, EXPOSURE, tile, THRESHOLD, DARK_LEVEL, MIN_SAMPLES, INTERVAL)
    c = np.array(r["counts"])
    assert len(c) == -(-W // tile) * -(-H // tile)
    hist = {int(k): int((c == k).sum()) for k in np.unique(c)}
    print("adaptive scene, tile", tile, ": observations -> tiles", hist)
    assert (c == MIN_SAMPLES).sum() >= 1  # frozen at the first check
    assert ((c > MIN_SAMPLES) & (c < SPP)).sum() >= 1  # frozen at a later check, before the end
    assert (c == SPP).sum() >= 1  # ran to spp_total
    assert hist == RECORDED_HIST[tile]
    # the border tiles (of the 8 x 8 list) see only void: no spread, frozen at once
    cm = adaptref.count_map(r, W, H, tile)
    assert tile != TILE or ((cm[0] == MIN_SAMPLES).all() and (cm[:, 0] == MIN_SAMPLES).all() and (cm[-1] == MIN_SAMPLES).all() and (cm[:, -1] == MIN_SAMPLES).all())
