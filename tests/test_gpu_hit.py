"""Hit reconstruction on the device (k_shade's fill_triangle / fill_curve, xform_normal / xform_point / xform_point_rel, the inverse of invert_affine) against
the float64 restatement in tests/hitref.py: the scenes and the check of tests/test_hit_cpu.py -- hitref's rays, hits, bounds, hit share and excluded share, all
taken before the renderer is looked at -- with skh_render_subframe as the renderer, under the options that change how a hit reaches its shading records.

Position and geometric normal.  The device has no path log, and none is added for this.  tests/test_hit_cpu.py::test_position_and_geometric_normal holds the
CHECKER's position and geometric normal against float64 through the origins of the rays that leave the first hit.  Here every scene's depth-4 render equals the
checker's bit for bit: the second ray of every path starts at offset_ray(position, geom_normal), so a device position or geometric normal that differed from the
checker's in one bit would start the bounce and the shadow ray elsewhere and move the pixel.  The checker's float64-checked values are thereby the device's."""
import numpy as np
import pytest

from strelka_amd import scene as S
from tests import test_hit_cpu as T
from tests.test_gpu_parity import _image_equal

pytestmark = pytest.mark.gpu

W, H = T.W, T.H


@pytest.fixture(scope="module")
def gpu():
    from strelka_amd import build

    build.build()


@pytest.fixture
def ctx(gpu):
    from strelka_amd import capi

    made = []

    def make(**options):
        c = capi.Context(0)
        made.append(c)
        for k, v in options.items():
            c.set_option(k, v)
        return c

    yield make
    for c in made:
        c.close()


def device_image(c, params):
    import torch

    img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    c.render_subframe(params, img.data_ptr())  # debug views go to the output image, not to the accumulator
    c.synchronize()
    return img.cpu().numpy()


def device_trace(c):
    return lambda o32, d32: c.trace(T.ray_records(o32, d32), 0)


OPTIONS = [{}, {"bake_world": 0}, {"direct_records": 0}, {"compact_hits": 0}]


@pytest.mark.parametrize("name", list(T.SCENES))
def test_normals_view_against_float64(ctx, name):
    """check_normals_view with the device as the renderer: default options; bake_world 0 (instances keep their top-level leaf, shading records are reached through
    the instance); direct_records 0; compact_hits 0; for the curve scenes world_kernel 0 as well"""
    build, texel, curves = T.SCENES[name]
    sc = build()
    arr, params = sc.arrays(), T.debug_params(sc)
    view = T.reference_view(arr, params)
    for opt in OPTIONS + ([{"world_kernel": 0}] if curves else []):
        c = ctx(**opt)
        c.set_scene(arr)
        c.resize(W, H)
        print(f"{name} {opt}:")
        T.check_normals_view(lambda p: device_image(c, p), arr, params, texel, device_trace(c), view)


@pytest.mark.parametrize("name", list(T.SCENES))
def test_normals_view_equals_the_checkers(ctx, name):
    build, texel, curves = T.SCENES[name]
    sc = build()
    arr, params = sc.arrays(), T.debug_params(sc)
    for bake in (None, 0):
        o = T.oracle_for(arr, bake)
        o.render_subframe(params)
        c = ctx(**({} if bake is None else {"bake_world": bake}))
        c.set_scene(arr)
        c.resize(W, H)
        want = o.read_image()
        assert (want[..., :3].sum(-1) > 0).mean() >= 0.4
        _image_equal(device_image(c, params), want)


@pytest.mark.parametrize("name", list(T.SCENES))
def test_depth_4_render_equals_the_checkers(ctx, name):
    """four sub-frames, depth 4: positions and geometric normals (module docstring)"""
    build, texel, curves = T.SCENES[name]
    sc = build()
    arr = sc.arrays()
    o = T.oracle_for(arr)
    c = ctx()
    c.set_scene(arr)
    c.resize(W, H)
    for i in range(4):
        p = S.frame_params(sc.getCamera(), W, H, subframe_index=i, spp_total=4, max_depth=4)
        o.render_subframe(p)
        c.render_subframe(p)
    want = o.read_accum()
    assert (want[..., :3].sum(-1) > 0).mean() > 0.1  # the scene is lit: the bounce and shadow rays count (a normal map that lays the normal into the surface leaves the least)
    _image_equal(c.read_accum(), want)
