"""oka::HipRender::setDenoiser on the device (tests/cpp/hiprender_denoise_main.cpp against the stand-in headers; INTEGRATION.md, "Denoiser"): with it on, every frame
is, byte for byte, what the ctypes path gives -- sub-frame, guide planes through the pixel centres, skh_denoise in place, tonemap --; with it off, what a HipRender
that never heard of it gives; and the guide planes are rendered once per accumulation restart."""
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 96, 64, 3


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from strelka_amd import build
    from tests.test_host_cpp import run_host

    tmp = tmp_path_factory.mktemp("hiprender_denoise")
    src, outd = tmp / "src", tmp / "out"
    src.mkdir()
    outd.mkdir()
    run_host(src, "cpu")  # the scene of host_test.cpp as a .skscene dump
    build.build_host()
    exe = str(tmp / "hiprender_denoise")
    host, lib = os.path.dirname(build.HOST_LIB), os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "hiprender_denoise_main.cpp"),
                           "-L" + host, "-loka_hip", "-L" + lib, "-lstrelka_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(outd), str(src / "scene.skscene"), str(FRAMES)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return outd


def image(outd, name):
    return np.fromfile(outd / name, np.float32).reshape(H, W, 4)


def test_off_is_a_render_that_never_heard_of_it(run):
    for f in range(FRAMES):
        assert (run / f"off_{f}.bin").read_bytes() == (run / f"plain_{f}.bin").read_bytes(), f
        assert (run / f"dn_{f}.bin").read_bytes() != (run / f"plain_{f}.bin").read_bytes(), f  # (and on, it filters)


def test_guides_once_per_accumulation(run):
    plain, off, on, moved, denoise_calls, subframe = (int(x) for x in open(run / "counts.txt").read().split())
    assert (plain, off) == (0, 0)  # no guide pass without the denoiser
    assert on == 1  # FRAMES frames of one accumulation: one guide pass
    assert moved == 2 and subframe == 2  # the camera moved: the accumulation restarted, one more guide pass for the two frames after it
    assert denoise_calls == FRAMES + 2


def test_on_gives_the_bits_of_the_ctypes_path(run):
    from strelka_amd import capi
    from tests.test_host_cpp import load as load_dump

    arr = load_dump(run)
    ap = np.fromfile(run / "aov_params.bin", S.AOV_PARAMS)[0]
    dp = np.fromfile(run / "denoise_params.bin", S.DENOISE_PARAMS)[0]
    exposure = S.default_exposure()
    # the mapping: four levels from 0, both flags, sigmaColor as given, the defaults for the rest
    assert [int(dp[k]) for k in ("width", "height", "first_level", "levels", "flags")] == [W, H, 0, 4, 3]
    assert float(dp["sigma_color"]) == np.float32(0.2) and float(dp["sigma_normal"]) == np.float32(0.3) and float(dp["albedo_floor"]) == np.float32(0.05)
    assert abs(float(dp["sigma_plane"]) / (S.DENOISE_PLANE_FRACTION * S.scene_diagonal(arr)) - 1.0) < 1e-6 and capi.denoise_check(dp)
    c = capi.Context(0)
    try:
        c.set_scene(arr)
        c.resize(W, H)
        d_image = c.buffer_alloc(16 * W * H)
        guides = c.render_guides(ap)
        bufs = {n: c.buffer_alloc(16 * W * H) for n in capi.DENOISE_GUIDES}
        for n, b in bufs.items():
            c.buffer_upload(b, guides[n])
        p = np.zeros((), S.FRAME_PARAMS)
        p["view_to_world"], p["clip_to_view"] = arr["camera"][:16], arr["camera"][16:]
        p["samples_this_launch"], p["spp_total"], p["max_depth"], p["enable_accumulation"] = 1, 64, 4, 1
        p["exposure"] = exposure
        got = np.zeros((H, W, 4), np.float32)
        for f in range(FRAMES):
            p["subframe_index"] = f
            c.render_subframe(p, d_image)
            c.denoise_device(dp, d_image, bufs["ids"], bufs["normal"], bufs["position"], bufs["albedo"], d_image)
            c.tonemap(d_image, W, H, 1, exposure, 2.4)
            c.buffer_download(d_image, got)
            assert got.tobytes() == (run / f"dn_{f}.bin").read_bytes(), f
        for b in list(bufs.values()) + [d_image]:
            c.buffer_free(b)
    finally:
        c.close()
