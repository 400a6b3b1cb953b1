"""oka::HipRender::setHistoryRectification on the device (tests/cpp/hiprender_rectify_render_main.cpp against the stand-in headers; INTEGRATION.md, "History
rectification"): with it off, every frame of the sequence still, move-instance, move-instance, still and every call count is what a HipRender that never heard
of it gives; with it on, a render() that reprojects a stored history makes exactly one more skh_temporal call and one skh_rectify call, and a render() that
continues an accumulation or has no history to reproject makes none."""
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 96, 64, 4
HAD = (0, 1, 1, 0)  # whether the frame's skh_temporal call reprojected a stored history: the first has none, the last continues an accumulation


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from strelka_amd import build
    from tests.test_host_cpp import run_host

    tmp = tmp_path_factory.mktemp("hiprender_rectify")
    src, outd = tmp / "src", tmp / "out"
    src.mkdir()
    outd.mkdir()
    run_host(src, "cpu")  # the scene of host_test.cpp as a .skscene dump
    build.build_host()
    exe = str(tmp / "hiprender_rectify_render")
    host, lib = os.path.dirname(build.HOST_LIB), os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "hiprender_rectify_render_main.cpp"), "-L" + host, "-loka_hip", "-L" + lib, "-lstrelka_hip",
                           "-Wl,-rpath," + host, "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(outd), str(src / "scene.skscene")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return outd


def calls(run, prefix):
    """per frame: (hadPrevious, skh_temporal, skh_rectify, skh_rewind_guides, skh_moments, skh_denoise calls so far)"""
    return [tuple(int(x) for x in line.split()) for line in open(run / f"{prefix}_calls.txt").read().strip().split("\n")]


def test_off_gives_the_images_and_the_call_counts_of_before(run):
    for f in range(FRAMES):
        assert (run / f"off_{f}.bin").read_bytes() == (run / f"plain_{f}.bin").read_bytes(), f
    plain = calls(run, "plain")
    assert calls(run, "off") == plain
    assert [c[0] for c in plain] == list(HAD) and [c[1] for c in plain] == [1, 2, 3, 4] and all(c[2] == 0 for c in plain)


def test_on_makes_one_more_temporal_call_and_one_rectify_call_per_reprojecting_render(run):
    plain, on = calls(run, "plain"), calls(run, "on")
    extra = np.cumsum(HAD)
    assert [c[0] for c in on] == list(HAD)
    assert [c[1] for c in on] == [plain[f][1] + int(extra[f]) for f in range(FRAMES)]  # skh_temporal: one more on frames 1 and 2, none on 0 and 3
    assert [c[2] for c in on] == [int(e) for e in extra]                               # skh_rectify: one on frames 1 and 2
    assert [c[3:] for c in on] == [c[3:] for c in plain]                               # the rewind, the moments and the denoiser are called as before
    # the first frame has no history to rectify and the last shows the accumulator: both are the plain pictures; the two between were clamped somewhere
    for f in (0, 3):
        assert (run / f"on_{f}.bin").read_bytes() == (run / f"plain_{f}.bin").read_bytes(), f
    assert any((run / f"on_{f}.bin").read_bytes() != (run / f"plain_{f}.bin").read_bytes() for f in (1, 2))
    words = np.fromfile(run / "on_rectify.bin", np.uint32)
    rec = np.frombuffer(words[:14].tobytes(), S.RECTIFY_PARAMS)[0]
    assert rec.tobytes() == S.rectify_params(W, H).tobytes() and words[14:].view(np.float32)[0] == np.float32(S.RECTIFY_FAST_HISTORY)


def test_on_in_the_guided_path_too(run):
    guided = calls(run, "ondn")
    extra = np.cumsum(HAD)
    assert [c[0] for c in guided] == list(HAD)
    assert [c[1] for c in guided] == [f + 1 + int(extra[f]) for f in range(FRAMES)] and [c[2] for c in guided] == [int(e) for e in extra]
    assert [c[4] for c in guided] == [1, 2, 3, 3]  # skh_moments on every call that starts an accumulation, as without the setting
    img = [np.fromfile(run / f"ondn_{f}.bin", np.float32) for f in range(FRAMES)]
    assert all(np.isfinite(i).all() for i in img)
