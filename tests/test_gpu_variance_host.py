"""oka::HipRender::setVarianceGuidance on the device (tests/cpp/hiprender_variance_main.cpp against the stand-in headers; INTEGRATION.md, "Variance guidance"):
with the setting off, every frame of the sequence still, still, move, move, still has the bits of a HipRender that never heard of it; with it on, a call that starts
an accumulation makes skh_temporal, skh_moments and skh_denoise_variance -- and is, byte for byte, what the ctypes path gives when it makes those calls --, a call
that continues one makes the calls it made before; without the denoiser the setting does not act; a resize drops the moments."""
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 96, 64, 5
STARTS = (True, False, True, True, True)  # still, still, move, move, still: which calls start an accumulation
SAMPLES = ((0, 1), (1, 1), (0, 0), (1, 0), (0, 1))
HAD_PREVIOUS = (0, 0, 1, 1, 1)
HAD_MOMENTS = (0, 0, 1, 1, 1)  # (frame 1 makes no guided call: the value of frame 0 stands)
LENGTHS = (1.0, 2.0, 1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from strelka_amd import build
    from tests.test_host_cpp import run_host

    tmp = tmp_path_factory.mktemp("hiprender_variance")
    src, outd = tmp / "src", tmp / "out"
    src.mkdir()
    outd.mkdir()
    run_host(src, "cpu")  # the scene of host_test.cpp as a .skscene dump
    build.build_host()
    exe = str(tmp / "hiprender_variance")
    host, lib = os.path.dirname(build.HOST_LIB), os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "hiprender_variance_main.cpp"),
                           "-L" + host, "-loka_hip", "-L" + lib, "-lstrelka_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(outd), str(src / "scene.skscene")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return outd


def test_off_is_a_render_that_never_heard_of_it(run):
    for f in range(FRAMES):
        assert (run / f"off_{f}.bin").read_bytes() == (run / f"tpdn_{f}.bin").read_bytes(), f
    # ... and on, the calls that start an accumulation give other pictures; the one that continues one gives the same
    assert (run / "vg_1.bin").read_bytes() == (run / "tpdn_1.bin").read_bytes()
    for f in (0, 2, 3, 4):
        assert (run / f"vg_{f}.bin").read_bytes() != (run / f"tpdn_{f}.bin").read_bytes(), f


def test_calls_per_frame_and_the_resize(run):
    plain_m, plain_v, off_m, off_v, alone_m, alone_v, after_resize, then = (int(x) for x in open(run / "counts.txt").read().split())
    assert (plain_m, plain_v, off_m, off_v) == (0, 0, 0, 0)  # without the setting: no new call
    assert (alone_m, alone_v) == (0, 0)  # without the denoiser the setting does not act
    assert (after_resize, then) == (0, 1)  # a resize drops the moments; the next start call has them again
    lines = [tuple(int(x) for x in line.split()) for line in open(run / "vg_calls.txt").read().strip().split("\n")]
    # subframe_index enable_accumulation hadPrevious hadPreviousMoments | skh_temporal skh_moments skh_denoise_variance skh_denoise calls of the frame
    want = [SAMPLES[f] + (HAD_PREVIOUS[f], HAD_MOMENTS[f]) + ((1, 1, 1, 0) if STARTS[f] else (1, 0, 0, 1)) for f in range(FRAMES)]
    assert lines == want


def test_on_gives_the_bits_of_the_ctypes_path(run):
    from strelka_amd import capi
    from tests.test_host_cpp import load as load_dump

    arr = load_dump(run)
    exposure = S.default_exposure()
    aov = [np.fromfile(run / f"vg_aov_{f}.bin", S.AOV_PARAMS)[0] for f in range(FRAMES)]
    applied = [np.fromfile(run / f"vg_temporal_{f}.bin", S.TEMPORAL_PARAMS)[0] for f in range(FRAMES)]
    variance = [np.fromfile(run / f"vg_variance_{f}.bin", S.VDENOISE_PARAMS)[0] for f in range(FRAMES)]
    dp = np.fromfile(run / "denoise_params.bin", S.DENOISE_PARAMS)[0]
    f32 = np.float32
    ex = np.asarray(exposure, f32)
    epsilon = f32(0.01) / f32(f32(f32(ex[0] + ex[1]) + ex[2]) / f32(3.0))
    c = capi.Context(0)
    try:
        c.set_scene(arr)
        c.resize(W, H)
        d_image = c.buffer_alloc(16 * W * H)
        guides = prev = prev_aov = moments = None
        got = np.zeros((H, W, 4), np.float32)
        for f in range(FRAMES):
            if STARTS[f]:
                # the filter's parameters are the denoiser's setting with the variance defaults and all three flags
                want = S.vdenoise_params(W, H, levels=int(dp["levels"]), sigma_normal=float(dp["sigma_normal"]), sigma_plane=dp["sigma_plane"],
                                         albedo_floor=float(dp["albedo_floor"]), epsilon=epsilon)
                assert variance[f].tobytes() == want.tobytes() and int(want["flags"]) == 7, f
                guides, stored_aov = c.render_guides(aov[f]), aov[f]
            p = np.zeros((), S.FRAME_PARAMS)
            p["view_to_world"], p["clip_to_view"] = aov[f]["view_to_world"], aov[f]["clip_to_view"]
            p["samples_this_launch"], p["spp_total"], p["max_depth"] = 1, 64, 4
            p["subframe_index"], p["enable_accumulation"] = SAMPLES[f]
            p["exposure"] = exposure
            c.render_subframe(p, d_image)
            image = np.zeros((H, W, 4), np.float32)
            c.buffer_download(d_image, image)
            out = c.temporal(image, guides, prev if HAD_PREVIOUS[f] else None, applied[f])
            if STARTS[f]:
                moments = c.moments(image, guides, out["motion"] if HAD_MOMENTS[f] else None, moments if HAD_MOMENTS[f] else None, applied[f])
                image = c.denoise_variance(out["image"], guides, moments, variance[f], moments_out=False)["image"]
            else:
                image = c.denoise(image, guides, dp)  # (a call that continues an accumulation: the accumulator's image, skh_denoise; the moments are left alone)
            prev = {"history": out["history"], "ids": guides["ids"], "normal": guides["normal"], "position": guides["position"]}
            prev_aov = stored_aov
            c.buffer_upload(d_image, image)
            c.tonemap(d_image, W, H, 1, exposure, 2.4)
            c.buffer_download(d_image, got)
            assert got.tobytes() == (run / f"vg_{f}.bin").read_bytes(), f
        c.buffer_free(d_image)
    finally:
        c.close()
