"""First-hit AOVs off the GPU ("First-hit AOVs"): the ABI's three symbols and the records' layout through the C compiler; skh_aov_check's
accept / refuse table through the binding and through a stand-alone program (tests/cpp/skhaov_main.cpp); scene.aov_params' matrices; and tests/aovref.py -- the
assembly of the expected planes -- against the CPU checker's normals view, before any device is involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from strelka_amd import build, capi, scene as S
from tests import aovref, hitref
from tests import test_hit_cpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = T.W, T.H


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# header <-> library <-> binding
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_layout(lib, tmp_path):
    for name in ("skh_aov_check", "skh_render_aovs", "skh_get_aov_info"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    for method in ("render_aovs", "render_aovs_device", "aov_info", "pick", "buffer_alloc", "buffer_free"):
        assert callable(getattr(capi.Context, method))
    dt = S.AOV_PARAMS
    assert dt.itemsize == 240 and dt.names == ("view_to_world", "clip_to_view", "world_to_clip", "x0", "y0", "width", "height", "sample_index", "spp_total", "tmin", "reserved")
    assert [dt.fields[n][1] for n in dt.names] == [0, 64, 128, 192, 196, 200, 204, 208, 212, 216, 220]
    assert capi.AOV_INFO.itemsize == 32 and [capi.AOV_INFO.fields[n][1] for n in capi.AOV_INFO.names] == [0, 8, 16, 24]
    fields = ("view_to_world", "clip_to_view", "world_to_clip", "x0", "y0", "width", "height", "sample_index", "spp_total", "tmin", "reserved")
    info = ("calls", "rays", "ms_last", "bytes_last")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strelka_hip.h"\nint main(void) { printf("%zu %zu", sizeof(skh_aov_params), sizeof(skh_aov_info));\n'
                   + "".join(f'printf(" %zu", offsetof(skh_aov_params, {f}));\n' for f in fields) + "".join(f'printf(" %zu", offsetof(skh_aov_info, {f}));\n' for f in info)
                   + 'printf(" %u %u %u %u %u %u %u %u %x\\n", SKH_AOV_IDS, SKH_AOV_HIT, SKH_AOV_NORMAL, SKH_AOV_POSITION, SKH_AOV_GEOM_NORMAL, SKH_AOV_ALBEDO, SKH_AOV_TEXCOORD, '
                   "SKH_AOV_COUNT, SKH_AOV_PIXEL_CENTRE); return SKH_ABI_VERSION == 5 ? 0 : 1; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0
    assert out.stdout.split() == [b"240", b"32"] + [str(dt.fields[n][1]).encode() for n in fields] + [b"0", b"8", b"16", b"24"] + [str(k).encode() for k in range(8)] + [b"ffffffff"]
    assert S.AOV_PLANES == ("ids", "hit", "normal", "position", "geom_normal", "albedo", "texcoord") and S.AOV_PIXEL_CENTRE == 0xFFFFFFFF
    assert "skh_aov.h" in [os.path.basename(d) for d in build.DEPS]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# skh_aov_check: one table for the binding and for the stand-alone program
# ---------------------------------------------------------------------------------------------------------------------------------------------
def good_params(**kw):
    cam = S.Camera(fov=40.0)
    cam.lookAt((1.0, 2.0, 5.0), (0.0, 0.5, 0.0))
    return S.aov_params(cam, W, H, **kw)


def edited(field, value, index=None, **kw):
    p = good_params(**kw)
    if index is None:
        p[field] = value
    else:
        p[field][index] = value
    return p


ACCEPTED = {"the whole image": good_params(), "the whole image, named": good_params(region=(0, 0, W, H)), "an interior region": good_params(region=(5, 3, 17, 11)),
            "a region that touches the right and bottom edge": good_params(region=(W - 9, H - 4, 9, 4)), "one pixel": good_params(region=(W - 1, H - 1, 1, 1)),
            "a sample": good_params(sample_index=63, spp_total=64), "tmin > 0": good_params(tmin=0.25)}
REFUSED = {"a region past the right edge": good_params(region=(W - 9, 0, 10, 4)), "a region past the bottom edge": good_params(region=(0, H - 3, 4, 4)),
           "an origin outside": good_params(region=(W, 0, 1, 1)), "a region that wraps": good_params(region=(2, 0, 0xFFFFFFFF, 1)),
           "zero width": good_params(region=(0, 0, 0, 4)), "zero height": good_params(region=(0, 0, 4, 0)), "the whole image from an origin": good_params(region=(1, 0, 0, 0)),
           "nan in view_to_world": edited("view_to_world", np.nan, 5), "inf in clip_to_view": edited("clip_to_view", np.inf, 0), "-inf in world_to_clip": edited("world_to_clip", -np.inf, 15),
           "tmin < 0": good_params(tmin=-1e-6), "tmin nan": good_params(tmin=np.nan), "tmin inf": good_params(tmin=np.inf),
           "spp_total 0": good_params(sample_index=0, spp_total=0), "sample_index == spp_total": good_params(sample_index=64, spp_total=64),
           "reserved[0]": edited("reserved", 1, 0), "reserved[4]": edited("reserved", 7, 4)}


def test_aov_check_accepts_and_refuses(lib):
    for name, p in ACCEPTED.items():
        assert capi.aov_check(p, W, H), name
    for name, p in REFUSED.items():
        assert not capi.aov_check(p, W, H), name
        assert lib.skh_aov_check(p.ctypes.data_as(C.c_void_p), W, H) == 3, name
    assert lib.skh_aov_check(None, W, H) == 3
    assert not capi.aov_check(good_params(), 0, 0)  # no image
    assert not capi.aov_check(good_params(region=(5, 3, 17, 11)), 21, 14) and capi.aov_check(good_params(region=(5, 3, 17, 11)), 22, 14)
    # pixel-centre mode ignores spp_total
    assert capi.aov_check(edited("spp_total", 0), W, H)


def test_aov_check_from_a_standalone_program(lib, tmp_path):
    """tests/cpp/skhaov_main.cpp: the C header and the library alone, the same table"""
    exe = str(tmp_path / "skhaov")
    libdir = os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "skhaov_main.cpp"),
                           "-L" + libdir, "-lstrelka_hip", "-Wl,-rpath," + libdir])
    cases = [(p, 0) for p in ACCEPTED.values()] + [(p, 3) for p in REFUSED.values()]
    lines = [f"{W} {H} " + " ".join("%08x" % w for w in np.frombuffer(p.tobytes(), np.uint32)) for p, _ in cases] + [f"{W} {H} NULL"]
    out = subprocess.run([exe], input="\n".join(lines).encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.decode().split("\n")
    assert got[0].split() == ["240", "32", "7", "ffffffff"]
    assert [int(x) for x in got[1:] if x] == [want for _, want in cases] + [3]


def test_aov_params_matrices():
    """the two matrices are frame_params'; world_to_clip inverts them: clip_to_view (world_to_clip (P, 1)) comes back to the view-space point, up to scale"""
    sc = T.flat_scene("rotation")
    cam = sc.getCamera()
    p, f = S.aov_params(cam, W, H), S.frame_params(cam, W, H)
    assert np.array_equal(p["view_to_world"], f["view_to_world"]) and np.array_equal(p["clip_to_view"], f["clip_to_view"])
    assert int(p["sample_index"]) == S.AOV_PIXEL_CENTRE and (int(p["width"]), int(p["height"])) == (0, 0) and not p["reserved"].any()
    v2w, c2v, w2c = (np.asarray(p[k], np.float64).reshape(4, 4) for k in ("view_to_world", "clip_to_view", "world_to_clip"))
    assert np.abs(w2c @ v2w @ c2v - np.eye(4)).max() < 1e-5
    # the camera looks down -z; with the projection Camera.updateAspectRatio writes, a point on the near plane has depth 0 and depth grows to 1 at the far plane --
    # the value the pass gives a miss
    eye, fwd = v2w[:3, 3], -v2w[:3, 2]
    d_near = aovref.depth64(p["world_to_clip"], (eye + cam.znear * fwd)[None])[0][0]
    d_mid = aovref.depth64(p["world_to_clip"], (eye + 500.0 * fwd)[None])[0][0]
    d_far = aovref.depth64(p["world_to_clip"], (eye + cam.zfar * fwd)[None])[0][0]
    assert abs(d_near) < 1e-4 and d_near < d_mid < d_far and abs(d_far - 1.0) < 1e-4
    q = S.aov_params(cam, W, H, region=(1, 2, 3, 4), sample_index=5, spp_total=16, tmin=0.5)
    assert [int(q[k]) for k in ("x0", "y0", "width", "height", "sample_index", "spp_total")] == [1, 2, 3, 4, 5, 16] and float(q["tmin"]) == 0.5


# ---------------------------------------------------------------------------------------------------------------------------------------------
# aovref against the checker
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_depth_bound_counts_roundings():
    """the float32 evaluation of mul44's two rows and the quotient, done here rounding by rounding, stays inside depth_bound of its float64 value"""
    sc = T.flat_scene("far")
    w2c = S.aov_params(sc.getCamera(), W, H)["world_to_clip"]
    rs = np.random.RandomState(5)
    v2w = np.asarray(S.aov_params(sc.getCamera(), W, H)["view_to_world"], np.float64).reshape(4, 4)
    P = (v2w[:3, 3] + rs.uniform(1.0, 40.0, (4000, 1)) * -v2w[:3, 2] + rs.normal(size=(4000, 3))).astype(np.float32)
    f = np.float32
    M = np.asarray(w2c, f).reshape(4, 4)
    row = lambda r: f(f(f(f(M[r, 0] * P[:, 0]) + f(M[r, 1] * P[:, 1])) + f(M[r, 2] * P[:, 2])) + f(M[r, 3] * f(1.0)))
    got = f(row(2) / row(3))
    bound, want = aovref.depth_bound(w2c, P)
    err = np.abs(got.astype(np.float64) - want)
    print(f"depth: max error / bound {(err / bound).max():.3f}, bound up to {bound.max():.2e}")
    assert (err <= bound).all() and (err / bound).max() > 0.02  # inside the bar, and the bar is not orders of magnitude too wide


@pytest.mark.parametrize("name", ["flat-rotation", "map-nonuniform-200-60-230", "curves-nonuniform"])
def test_assembled_planes_against_the_checkers_normals_view(name):
    """T.check_normals_view with, as the renderer, the planes aovref assembles from the checker's own trace() of sample 0's rays: the assembly indexes pixels,
    instances, records and materials correctly -- and the checker's own view equals what it shows, within float32's rounding of the image"""
    builder, texel, curves = T.SCENES[name]
    sc = builder()
    arr, params = sc.arrays(), T.debug_params(sc)
    o = T.oracle_for(arr)
    ro, rd = hitref.camera_rays(params, W, H, 0, T.jitter())
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    rec = o.trace(T.ray_records(ro, rd), 0)
    w2c = S.aov_params(sc.getCamera(), W, H)["world_to_clip"]
    want = aovref.assemble(arr, ro, rd, rec, w2c)
    kind = want["ids"][:, 3]
    assert (kind == aovref.KIND_LIGHT).sum() == 0 and (kind == aovref.KIND_MISS).any() == (not curves)  # (the curve scenes' backdrop fills the frame)
    assert ((kind == aovref.KIND_CURVE).sum() > 400) == curves
    view = aovref.normals_view(want["normal"], kind).reshape(H, W, 3)
    T.check_normals_view(lambda p: view, arr, params, texel, T.oracle_trace(o, params) if curves else (lambda o32, d32: o.trace(T.ray_records(o32, d32), 0)))
    # the checker's image of the same pixels: equal up to the roundings of its own float32 chain, which check_normals_view has just bounded for both
    img = T.oracle_render(o)(params)[..., :3].reshape(-1, 3)
    surf = (kind == aovref.KIND_TRIANGLE) | (kind == aovref.KIND_CURVE)
    assert (img[kind == aovref.KIND_MISS] == 0).all()
    tri = kind == aovref.KIND_TRIANGLE  # (a curve's end caps have a rule of their own: check_normals_view leaves them out, and so does this line)
    assert np.abs(img[tri].astype(np.float64) - view.reshape(-1, 3)[tri]).max() < 1e-5
    # ids, facing and depth of the assembly
    assert (want["ids"][kind == aovref.KIND_MISS] == [aovref.MISS, aovref.MISS, aovref.MISS, 0]).all() and (want["hit"][kind == aovref.KIND_MISS] == [-1, 0, 0]).all()
    assert (want["facing"][surf] != 0).all() and (want["facing"][kind == aovref.KIND_TRIANGLE] == 1).all()  # the scenes are seen from the side their normals name
    assert (want["depth"][kind == aovref.KIND_MISS] == 1).all() and (want["depth"][surf] > 0).all() and (want["depth"][surf] < 1).all()
    mats = want["ids"][surf, 2]
    assert set(np.unique(mats)) <= set(range(len(arr["materials"]))) and (want["ids"][~surf, 2] == aovref.MISS).all()
