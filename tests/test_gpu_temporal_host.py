"""oka::HipRender::setTemporal on the device (tests/cpp/hiprender_temporal_main.cpp against the stand-in headers; INTEGRATION.md, "Temporal accumulation"): with it
off, every frame is what a HipRender that never heard of it gives; with it on, every frame of the sequence still, still, move, move, still is, byte for byte, what
the ctypes path gives when it makes the calls the header prescribes -- the guide pass once per accumulation, the rotated raw sample on the moving calls, the
reprojection on the calls that start an accumulation, the seeding call on those that continue one, then skh_denoise when that is on, then the tonemap."""
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 96, 64, 5
STARTS = (True, False, True, True, True)  # still, still, move, move, still: which calls start an accumulation
SAMPLES = ((0, 1), (1, 1), (0, 0), (1, 0), (0, 1))  # (subframe_index, enable_accumulation): the moving calls take raw samples 0, 1, ... of the sequence
HAD_PREVIOUS = (0, 0, 1, 1, 1)
LENGTHS = (1.0, 2.0, 1.0, 1.0, 1.0)  # initial_length: the seeding call of frame 1 stores the accumulator with its two samples


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from strelka_amd import build
    from tests.test_host_cpp import run_host

    tmp = tmp_path_factory.mktemp("hiprender_temporal")
    src, outd = tmp / "src", tmp / "out"
    src.mkdir()
    outd.mkdir()
    run_host(src, "cpu")  # the scene of host_test.cpp as a .skscene dump
    build.build_host()
    exe = str(tmp / "hiprender_temporal")
    host, lib = os.path.dirname(build.HOST_LIB), os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "hiprender_temporal_main.cpp"),
                           "-L" + host, "-loka_hip", "-L" + lib, "-lstrelka_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(outd), str(src / "scene.skscene")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return outd


def test_off_is_a_render_that_never_heard_of_it(run):
    for f in range(FRAMES):
        assert (run / f"off_{f}.bin").read_bytes() == (run / f"plain_{f}.bin").read_bytes(), f
    # ... and on, the frames that reproject a history are other pictures.  Frame 1 continues an accumulation and shows the accumulator's image: the plain one's
    # bytes.  Frame 0 has no history and is the plain one up to the rounding of (C / m) m, the definition's d_out for a pixel without history.
    assert (run / "tp_1.bin").read_bytes() == (run / "plain_1.bin").read_bytes()
    first, plain = (np.fromfile(run / name, np.float32) for name in ("tp_0.bin", "plain_0.bin"))
    assert np.abs(first - plain).max() <= 1e-6  # (tonemapped values in [0, 1])
    for f in (2, 3, 4):
        assert (run / f"tp_{f}.bin").read_bytes() != (run / f"plain_{f}.bin").read_bytes(), f


def test_counts(run):
    guides, calls, guides_after, calls_after, had_after, plain_guides, plain_calls, off_guides, off_calls, subframe = (int(x) for x in open(run / "counts.txt").read().split())
    assert (plain_guides, plain_calls, off_guides, off_calls) == (0, 0, 0, 0)  # without the feature: no guide pass, no call
    assert calls == FRAMES  # exactly one skh_temporal per render()
    assert guides == sum(STARTS)  # one guide pass per accumulation, none for the frame that continues one
    assert (guides_after, calls_after, had_after) == (guides + 1, calls + 1, 0)  # a new sky: the accumulation restarts without a previous frame
    assert subframe == 1
    for prefix in ("tp", "tpdn"):
        lines = [tuple(int(x) for x in line.split()) for line in open(run / f"{prefix}_calls.txt").read().strip().split("\n")]
        assert lines == [SAMPLES[f] + (HAD_PREVIOUS[f],) for f in range(FRAMES)], prefix


@pytest.mark.parametrize("prefix", ["tp", "tpdn"])
def test_on_gives_the_bits_of_the_ctypes_path(run, prefix):
    from strelka_amd import capi
    from tests.test_host_cpp import load as load_dump

    arr = load_dump(run)
    exposure = S.default_exposure()
    aov = [np.fromfile(run / f"{prefix}_aov_{f}.bin", S.AOV_PARAMS)[0] for f in range(FRAMES)]
    applied = [np.fromfile(run / f"{prefix}_temporal_{f}.bin", S.TEMPORAL_PARAMS)[0] for f in range(FRAMES)]
    dp = np.fromfile(run / "denoise_params.bin", S.DENOISE_PARAMS)[0] if prefix == "tpdn" else None
    assert not np.array_equal(aov[1]["view_to_world"], aov[2]["view_to_world"]) and not np.array_equal(aov[2]["view_to_world"], aov[3]["view_to_world"])
    assert np.array_equal(aov[0]["view_to_world"], aov[1]["view_to_world"]) and np.array_equal(aov[3]["view_to_world"], aov[4]["view_to_world"])
    c = capi.Context(0)
    try:
        c.set_scene(arr)
        c.resize(W, H)
        d_image = c.buffer_alloc(16 * W * H)
        guides = prev = prev_aov = None
        got = np.zeros((H, W, 4), np.float32)
        for f in range(FRAMES):
            # the parameters HipRender handed over are the mapping of the defaults, with the matrix of the stored guide set and the prescribed length
            plane = float(applied[f]["plane_tolerance"])
            want = S.temporal_params(W, H, prev_aov if HAD_PREVIOUS[f] else None, plane_tolerance=plane, initial_length=LENGTHS[f])
            assert applied[f].tobytes() == want.tobytes() and abs(plane / (S.DENOISE_PLANE_FRACTION * S.scene_diagonal(arr)) - 1.0) < 1e-6, f
            if STARTS[f]:
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
                image = out["image"]  # (a call that continues an accumulation shows the accumulator's image)
            prev = {"history": out["history"], "ids": guides["ids"], "normal": guides["normal"], "position": guides["position"]}
            prev_aov = stored_aov
            if dp is not None:
                image = c.denoise(image, guides, dp)
            c.buffer_upload(d_image, image)
            c.tonemap(d_image, W, H, 1, exposure, 2.4)
            c.buffer_download(d_image, got)
            assert got.tobytes() == (run / f"{prefix}_{f}.bin").read_bytes(), f
        c.buffer_free(d_image)
    finally:
        c.close()
