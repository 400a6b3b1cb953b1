"""oka::HipRender::setInstanceMotion on the device (tests/cpp/hiprender_motion_main.cpp against the stand-in headers; INTEGRATION.md, "Object motion"): with it
off, every frame of the sequence still, move-instance, move-instance, still is what a HipRender that never heard of it gives; with it on, every frame is, byte
for byte, what the ctypes path gives when it makes the calls INTEGRATION.md prescribes -- skh_update_accel, the guide pass, the sample, then on a call that
reprojects across a transform change the table from the C helper, skh_set_instance_motion, one skh_rewind_guides, and skh_temporal on the rewound normal and
position planes; skh_denoise on the true ones; the tonemap.  With variance guidance on as well, skh_moments takes the rewound position and
skh_denoise_variance the true planes."""
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 96, 64, 4
STARTS = (True, True, True, False)  # still, move-instance, move-instance, still: which calls start an accumulation
REWINDS = (0, 1, 2, 2)  # skh_rewind_guides calls so far: one per call that reprojects across a transform change
CALLS = ((0, 1, 0), (0, 1, 1), (0, 1, 1), (1, 1, 0))  # subframe_index, enable_accumulation, hadPrevious: the camera is at rest, no raw samples


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from strelka_amd import build
    from tests.test_host_cpp import run_host

    tmp = tmp_path_factory.mktemp("hiprender_motion")
    src, outd = tmp / "src", tmp / "out"
    src.mkdir()
    outd.mkdir()
    run_host(src, "cpu")  # the scene of host_test.cpp as a .skscene dump
    build.build_host()
    exe = str(tmp / "hiprender_motion")
    host, lib = os.path.dirname(build.HOST_LIB), os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "hiprender_motion_main.cpp"),
                           "-L" + host, "-loka_hip", "-L" + lib, "-lstrelka_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(outd), str(src / "scene.skscene")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return outd


def test_off_is_a_render_that_never_heard_of_it_and_on_is_another_picture(run):
    for f in range(FRAMES):
        assert (run / f"off_{f}.bin").read_bytes() == (run / f"plain_{f}.bin").read_bytes(), f
    # on: the frames that reproject across a move are other pictures; the first frame and the one that continues an accumulation are the plain ones
    for f in (0, 3):
        assert (run / f"mo_{f}.bin").read_bytes() == (run / f"plain_{f}.bin").read_bytes(), f
    for f in (1, 2):
        assert (run / f"mo_{f}.bin").read_bytes() != (run / f"plain_{f}.bin").read_bytes(), f


def test_counts(run):
    plain_calls, plain_entries, off_calls, off_entries, mo_calls, mo_entries, modn_calls, modn_entries, movg_calls, movg_entries = (
        int(x) for x in open(run / "counts.txt").read().split())
    assert (plain_calls, plain_entries, off_calls, off_entries) == (0, 0, 0, 0)  # without the feature: no call, no table
    n = len(np.fromfile(run / "instances.bin", S.INSTANCE))
    assert (mo_calls, mo_entries, modn_calls, modn_entries, movg_calls, movg_entries) == (REWINDS[-1], n) * 3
    for prefix in ("mo", "modn", "movg"):
        lines = [tuple(int(x) for x in line.split()) for line in open(run / f"{prefix}_calls.txt").read().strip().split("\n")]
        assert lines == [CALLS[f] + (REWINDS[f],) for f in range(FRAMES)], prefix  # exactly one rewind per render() that reprojects across a move, none otherwise


@pytest.mark.parametrize("prefix", ["mo", "modn", "movg"])
def test_on_gives_the_bits_of_the_ctypes_path(run, prefix):
    from strelka_amd import capi
    from tests.test_host_cpp import load as load_dump

    arr = load_dump(run)
    exposure = S.default_exposure()
    aov = [np.fromfile(run / f"{prefix}_aov_{f}.bin", S.AOV_PARAMS)[0] for f in range(FRAMES)]
    applied = [np.fromfile(run / f"{prefix}_temporal_{f}.bin", S.TEMPORAL_PARAMS)[0] for f in range(FRAMES)]
    instances = [np.fromfile(run / f"{prefix}_instances_{f}.bin", S.INSTANCE) for f in range(FRAMES)]
    dp = np.fromfile(run / "denoise_params.bin", S.DENOISE_PARAMS)[0] if prefix != "mo" else None
    variance = [np.fromfile(run / f"movg_variance_{f}.bin", S.VDENOISE_PARAMS)[0] for f in range(FRAMES)] if prefix == "movg" else None
    assert np.array_equal(instances[0], arr["instances"]) and np.array_equal(instances[2], instances[3])
    assert not np.array_equal(instances[0]["transform"], instances[1]["transform"]) and not np.array_equal(instances[1]["transform"], instances[2]["transform"])
    assert all(np.array_equal(aov[0]["view_to_world"], aov[f]["view_to_world"]) for f in range(FRAMES))  # (the camera is at rest)
    c = capi.Context(0)
    try:
        c.set_scene(arr)
        c.resize(W, H)
        d_image = c.buffer_alloc(16 * W * H)
        guides = prev = guide_instances = prev_guide_instances = moments = None
        got = np.zeros((H, W, 4), np.float32)
        rewinds = 0
        for f in range(FRAMES):
            if f and not np.array_equal(instances[f]["transform"], instances[f - 1]["transform"]):
                c.update_accel(instances[f])
            if STARTS[f]:
                guides = c.render_guides(aov[f])
                prev_guide_instances, guide_instances = guide_instances, instances[f]
            p = np.zeros((), S.FRAME_PARAMS)
            p["view_to_world"], p["clip_to_view"] = aov[f]["view_to_world"], aov[f]["clip_to_view"]
            p["samples_this_launch"], p["spp_total"], p["max_depth"] = 1, 64, 4
            p["subframe_index"], p["enable_accumulation"] = CALLS[f][:2]
            p["exposure"] = exposure
            c.render_subframe(p, d_image)
            image = np.zeros((H, W, 4), np.float32)
            c.buffer_download(d_image, image)
            had = bool(CALLS[f][2])
            current = guides
            if STARTS[f] and had and not np.array_equal(guide_instances["transform"], prev_guide_instances["transform"]):
                c.set_instance_motion(S.instance_motion(prev_guide_instances, guide_instances))
                rw = c.rewind_guides(guides)
                current = dict(guides, position=rw["position"], normal=rw["normal"])
                rewinds += 1
            assert rewinds == REWINDS[f] == c.rewind_info()["calls"]
            out = c.temporal(image, current, prev if had else None, applied[f])
            prev = {"history": out["history"], "ids": guides["ids"], "normal": guides["normal"], "position": guides["position"]}  # (the TRUE planes are stored)
            if variance is not None and STARTS[f]:
                # a guided call: the moments through the rewound position and that call's motion plane, the filter on the true planes
                moments = c.moments(image, current, out["motion"] if had else None, moments if had else None, applied[f])
                image = c.denoise_variance(out["image"], guides, moments, variance[f], moments_out=False)["image"]
            else:
                if STARTS[f]:
                    image = out["image"]  # (a call that continues an accumulation shows the accumulator's image)
                if dp is not None:
                    image = c.denoise(image, guides, dp)
            c.buffer_upload(d_image, image)
            c.tonemap(d_image, W, H, 1, exposure, 2.4)
            c.buffer_download(d_image, got)
            assert got.tobytes() == (run / f"{prefix}_{f}.bin").read_bytes(), f
        c.buffer_free(d_image)
    finally:
        c.close()
