"""CPU-side checks of the environment light's plumbing: the Radiance .hdr reader / writer, the three C-ABI symbols and their Python binding,
`Scene.setEnvironment` / `arrays()`, and the float64 restatement the GPU tests compare against (tests/envref.py) against closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from strelka_amd import hdr, scenes
from tests import envref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _picture(seed=3, h=24, w=70):
    rs = np.random.RandomState(seed)
    img = (rs.rand(h, w, 3) ** 6 * 5e3).astype(np.float32)
    img[4:11, 9:60] = (2.5, 0.125, 7.0)  # long runs in every byte plane
    img[0, :5] = 0.0
    img[h // 2, 3] = (1e-38, 0, 0)  # below the format's range: reads as black
    return img


@pytest.mark.parametrize("rle", [True, False])
def test_hdr_round_trip_reproduces_the_rgbe_quantised_data(tmp_path, rle):
    img = _picture()
    want = hdr.rgbe_quantise(img)
    # RGBE keeps 8 bits of the LARGEST channel: relative to it nothing is further than 2^-8 away
    assert (np.abs(want - img).max(axis=-1) <= img.max(axis=-1) / 256 + 1e-37).all() and want[12, 3].max() == 0
    path = str(tmp_path / "a.hdr")
    hdr.save_hdr(path, img, rle=rle)
    got = hdr.load_hdr(path)
    assert got.dtype == np.float32 and got.shape == img.shape and np.array_equal(got, want)
    assert np.array_equal(hdr.rgbe_quantise(got), got)  # a fixed point: a second trip changes nothing
    data = open(path, "rb").read()
    assert data.startswith(b"#?RADIANCE\n") and b"\n-Y 24 +X 70\n" in data
    if rle:
        assert len(data) < len(hdr.encode_hdr(img, rle=False))  # the runs were found
    narrow = img[:, :5]  # below 8 texels a scanline is always flat
    assert np.array_equal(hdr.decode_hdr(hdr.encode_hdr(narrow, rle=rle)), hdr.rgbe_quantise(narrow))


def test_hdr_reads_both_encodings_mixed_and_refuses_bad_files():
    img = _picture(5, 6, 16)
    flat, rle = hdr.encode_hdr(img, rle=False), hdr.encode_hdr(img, rle=True)
    assert np.array_equal(hdr.decode_hdr(flat), hdr.decode_hdr(rle))
    for data in (flat, rle):
        for cut in (len(data) - 1, len(data) - 40, data.find(b"+X") + 8):
            with pytest.raises(hdr.HdrError):
                hdr.decode_hdr(data[:cut])
    with pytest.raises(hdr.HdrError, match="signature"):
        hdr.decode_hdr(b"P6\n" + flat[3:])
    with pytest.raises(hdr.HdrError, match="FORMAT"):
        hdr.decode_hdr(flat.replace(b"32-bit_rle_rgbe", b"32-bit_rle_xyze"))
    with pytest.raises(hdr.HdrError, match="orientation"):
        hdr.decode_hdr(flat.replace(b"-Y 6 +X 16", b"+Y 6 +X 16"))
    with pytest.raises(hdr.HdrError):
        hdr.decode_hdr(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n")  # the header never ends
    bad = bytearray(rle)
    k = rle.find(b"+X 16\n") + 6
    bad[k + 4] = 128 + 100  # a run longer than the scanline
    with pytest.raises(hdr.HdrError):
        hdr.decode_hdr(bytes(bad))
    with pytest.raises(hdr.HdrError):
        hdr.encode_hdr(np.full((4, 4, 3), -1.0, np.float32))


def test_environment_symbols_are_declared_exported_and_bound():
    from strelka_amd import build, capi

    build.build()
    lib = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "strelka_hip.h")).read(), flags=re.S)
    for name in ("skh_set_environment", "skh_set_environment_transform", "skh_get_environment_info"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert "typedef struct skh_environment" in header and re.search(r"SKH_UNIT_ENV_SAMPLE = 9,\s*SKH_UNIT_ENV_EVAL = 10,\s*SKH_UNIT_COUNT = 11", header)
    assert capi.Context.UNITS["env_sample"] == (9, 2, 9) and capi.Context.UNITS["env_eval"] == (10, 3, 6)
    assert C.sizeof(capi.SkhEnvironment) == 8 + 8 + 12 + 36 and capi.ENVIRONMENT_INFO.itemsize == 32
    # null-context calls are refused, not crashed
    e = capi.SkhEnvironment()
    info = np.zeros((), capi.ENVIRONMENT_INFO)
    z = np.zeros(9, np.float32)
    assert lib.skh_set_environment(None, C.byref(e)) != 0
    assert lib.skh_set_environment_transform(None, z.ctypes.data, z.ctypes.data) != 0
    assert lib.skh_get_environment_info(None, info.ctypes.data) != 0
    assert lib.skh_last_error(None) == b"null context"


def test_scene_arrays_carry_an_environment_only_when_one_is_set():
    sc = scenes.cornell_box()
    keys = {"vertices", "indices", "meshes", "curves", "curve_points", "curve_radii", "curve_vertex_counts", "instances", "lights", "materials", "textures"}
    assert set(sc.arrays().keys()) == keys
    rgb = envref.sky_map(16, 8, 1)
    sc.setEnvironment(rgb, scale=(2, 2, 2))
    arr = sc.arrays()
    assert set(arr.keys()) == keys | {"environment"}
    env = arr["environment"]
    assert np.array_equal(env["rgb"], rgb) and env["rgb"].dtype == np.float32 and np.array_equal(env["world_to_env"], np.eye(3, dtype=np.float32))
    assert np.array_equal(env["scale"], np.float32([2, 2, 2]))
    sc.setEnvironment(None)
    assert set(sc.arrays().keys()) == keys
    with pytest.raises(ValueError):
        sc.setEnvironment(np.zeros((4, 4), np.float32))
    # the CPU checker knows no environment and ignores the entry
    from tests import orklib

    sc.setEnvironment(rgb)
    o = orklib.new_context()
    o.set_scene(sc.arrays())


def test_reference_restatement_against_closed_forms():
    """tests/envref.py is what the GPU tests trust: a constant map's pdf is 1 / 4 pi up to the row-centre quadrature of sin, its cosine moments are the
    constant and its square, the CDFs end at 1, and the texel of a texel centre's direction is that texel."""
    W, H = 64, 32
    const = np.full((H, W, 3), 0.25, np.float32)
    d = envref.random_directions(2000, 4)
    ix, iy = envref.texel_of(d, W, H)
    p = envref.pdf(const, d, ix, iy)
    sin_th = np.hypot(d[:, 0].astype(np.float64), d[:, 2].astype(np.float64))  # (not sin(acos(y)): that loses its digits at the poles)
    centre = np.sin(np.pi * (iy + 0.5) / H)
    want = centre / sin_th / (4 * np.pi) * np.sin(np.pi / (2 * H)) / (np.pi / (2 * H))  # sum over rows of sin(centre) = 1 / sin(pi / 2H)
    assert np.allclose(p, want, rtol=1e-6)
    m1, m2 = envref.cosine_moments(const, (2, 1, 4))
    assert np.allclose(m1, [0.5, 0.25, 1.0], rtol=1e-12) and np.allclose(m2, [0.25, 0.0625, 1.0], rtol=1e-12)
    sky = envref.sky_map(W, H, 7)
    marg, cond, total = envref.cdfs(sky)
    assert marg[0] == 0 and abs(marg[-1] - 1) < 1e-12 and np.allclose(cond[:, -1], 1, atol=1e-12) and (np.diff(marg) > 0).all() and total > 0
    assert sky.max() / np.median(sky) > 1e3  # the sun is there
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    t, f = np.pi * (yy.ravel() + 0.5) / H, 2 * np.pi * (xx.ravel() + 0.5) / W
    dirs = np.stack([np.sin(t) * np.cos(f), np.cos(t), np.sin(t) * np.sin(f)], 1)
    gx, gy = envref.texel_of(dirs, W, H)
    assert np.array_equal(gx, xx.ravel()) and np.array_equal(gy, yy.ravel())
    # a quarter turn about Y moves phi by a quarter of the map
    R = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)
    rx, ry = envref.texel_of(dirs, W, H, R)
    assert np.array_equal(ry, gy) and len(set(((rx - gx) % W).tolist())) == 1


def test_the_adapter_has_the_method_and_the_mirror_of_the_reference_headers_does_not():
    """`HipRender::setEnvironment` is a method of the subclass only: strelka_amd/host/oka_mirror.* restates the reference's headers, which know no dome light."""
    h = open(os.path.join(ROOT, "integration", "HipRender.h")).read()
    c = open(os.path.join(ROOT, "integration", "HipRender.cpp")).read()
    assert "bool setEnvironment(const float* rgb, uint32_t width, uint32_t height, const float scale[3], const float* worldToEnv" in h
    assert "skh_set_environment(mCtx" in c and "skh_set_environment_transform(mCtx" in c
    for f in ("oka_mirror.h", "oka_mirror.cpp", "oka_render.h"):
        assert "nvironment" not in open(os.path.join(ROOT, "strelka_amd", "host", f)).read(), f
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "domeLight" in doc and "setEnvironment" in doc
