"""Derived state follows its inputs (strelka_amd/csrc/skh_stale.h; the matrix itself: tests/test_stale_table.py).  One case per row of the table that
invalidates something: a context renders scene X, takes the row's change -- one setter call -- and renders again; image and derived tables must be those of a
fresh context that was given the changed scene Y from the start.  The row of an in-place update that fails half way cannot be reached without a failing HIP
call and is held by the matrix test alone.  32 x 32 pixels, 1 spp, depth 2: a floor, an emissive quad, a textured card with a cutout entry, a rect light and
a sampled disk light (a light-shape entry); the curve case adds eight strands."""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from tests import blendref, cutref

pytestmark = pytest.mark.gpu

W = H = 32
RECT_XF = S.translate((0.0, 3.0, 0.0)) @ S.rotate((1, 0, 0), math.radians(-90))  # a rect light emits along local -Z
DISK_XF = S.translate((1.2, 2.5, 0.0)) @ S.rotate((1, 0, 0), math.radians(90))  # a disk's normal is its local +Z
EMIT_XF = S.translate((-1.2, 2.6, 0.0))
EMIT_XF_MOVED = S.translate((-0.9, 2.4, 0.2)) @ S.scale((1.5, 1.0, 0.5))  # (another area: another sum of weights)


def build(emit_half=0.4, emit_xf=EMIT_XF, card_material=2, alpha_phase=0, floor_rgb=(0.6, 0.6, 0.6), curves=False, curve_dx=0.0):
    sc = S.Scene()
    a = np.zeros((8, 8, 4), np.uint8)
    a[..., :3] = (200, 160, 120)
    yy, xx = np.mgrid[0:8, 0:8]
    a[..., 3] = np.where((xx // 2 + yy // 2 + alpha_phase) % 2 == 0, 255, 0)
    tex = sc.addTexture(a)
    grey = sc.addMaterial(S.MAT_DIFFUSE, floor_rgb)
    lamp = sc.addMaterial(S.MAT_DIFFUSE, (0.1, 0.1, 0.1), emission=(6.0, 5.0, 4.0))
    card = sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6), base_color_texture=tex, opacity_texture=tex, opacity_channel=3, opacity_threshold=0.5)
    assert (grey, lamp, card) == (0, 1, 2)
    sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)]), grey, np.eye(4))
    e = emit_half
    sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-e, 0, -0.5), (e, 0, -0.5), (e, 0, 0.5), (-e, 0, 0.5)]), lamp, emit_xf)  # faces down
    sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-0.6, 0, 0.6), (0.6, 0, 0.6), (0.6, 0, -0.6), (-0.6, 0, -0.6)], uv=[(0, 0), (1, 0), (1, 1), (0, 1)]),
                      card_material, S.translate((0.3, 1.0, 0.0)))
    if curves:
        hair = sc.addHairMaterial((0.35, 0.2, 0.1))
        t = np.linspace(-0.2, 1.2, 8)[None, :, None]  # (the first and last control points are the phantom points of the strand)
        root = np.stack([np.linspace(-1.0, -0.3, 8) + curve_dx, np.zeros(8), np.linspace(0.9, 0.2, 8)], 1)[:, None, :]
        pts = root + t * np.array([0.1, 0.9, 0.0])[None, None, :]
        cid = sc.createCurve(np.full(8, 8, np.uint32), pts.reshape(-1, 3), np.full(64, 0.02, np.float32))
        sc.createInstance(S.INSTANCE_CURVE, cid, hair, np.eye(4))
    sc.createLight({"type": 0, "xform": RECT_XF, "useXform": True, "width": 1.5, "height": 1.5, "color": (10.0, 10.0, 10.0), "intensity": 1.0})
    sc.createLight({"type": 1, "xform": DISK_XF, "useXform": True, "radius": 0.4, "color": (10.0, 6.0, 3.0), "intensity": 1.0, "sample": True})
    sc.addCamera(cutref.camera())
    return sc


def make_ctx(arr, options=None):
    from strelka_amd import build as B, capi

    B.build()
    c = capi.Context(0)
    for k, v in (options or {}).items():
        c.set_option(k, v)
    c.set_scene(arr)
    return c


def render(c, cam):
    c.resize(W, H)
    c.render_subframe(S.frame_params(cam, W, H, subframe_index=0, samples_this_launch=1, spp_total=1, max_depth=2))
    return c.read_accum()


def derived(c, n_instances):
    e, cu, b = c.emitter_info(), c.cutout_info(), c.blend_info()
    return {"emitter": (e["triangles"], e["instances"], e["sum_w"]), "cutout": (cu["active_materials"], cu["instances"]),
            "blend": (b["active_materials"], b["instances"]), "light_shapes": c.light_shape_info(), "baked": c.baked(n_instances)[1:]}


def without(arr, key):
    return {k: v for k, v in arr.items() if k != key}


def cone_on_the_rect(arr):
    ls = arr["light_shapes"].copy()
    assert len(ls) == 2 and int(ls[1]["flags"]) == S.LIGHT_SHAPE_SAMPLE_DISC
    ls[1]["flags"] = 0
    ls[0]["flags"], ls[0]["cos_outer"], ls[0]["cos_inner"], ls[0]["axis"] = S.LIGHT_SHAPE_CONE, math.cos(math.radians(40)), math.cos(math.radians(30)), (0.0, -1.0, 0.0)
    return ls


def floor_emits(arr):
    em = arr["emission"].copy()
    em[0], em[1] = (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)
    return em


# name -> (scene X's arguments, Y's arrays from X's, the row's one call, options of both contexts after the change)
CASES = {
    "set_geometry": ({}, lambda x: build(emit_half=0.6).arrays(), lambda c, y: c.set_geometry(y), {}),
    "set_curves": ({"curves": True}, lambda x: build(curves=True, curve_dx=0.25).arrays(), lambda c, y: c.set_curves(y), {}),
    "set_instances": ({}, lambda x: build(emit_xf=EMIT_XF_MOVED, card_material=0).arrays(), lambda c, y: c.set_instances(y["instances"]), {}),
    "set_lights": ({}, lambda x: dict(x, lights=x["lights"][::-1].copy()), lambda c, y: c.set_lights(y["lights"]), {}),  # (the disk's shape entry now meets the rect)
    "set_textures": ({}, lambda x: build(alpha_phase=1).arrays(), lambda c, y: c.set_textures(y["textures"]), {}),
    "set_materials": ({}, lambda x: build(floor_rgb=(0.2, 0.5, 0.7)).arrays(), lambda c, y: c.set_materials(y["materials"]), {}),
    "set_emission": ({}, lambda x: dict(x, emission=floor_emits(x)), lambda c, y: c.set_emission(y["emission"]), {}),
    "set_emission_removed": ({}, lambda x: without(x, "emission"), lambda c, y: c.set_emission(None), {}),
    "set_material_cutouts": ({}, lambda x: dict(x, material_cutouts=cutref.table(len(x["materials"]), {})), lambda c, y: c.set_material_cutouts(y["material_cutouts"]), {}),
    "set_material_blend": ({}, lambda x: dict(x, material_blend=blendref.table(len(x["materials"]), {0: blendref.constant(0.5)})),
                           lambda c, y: c.set_material_blend(y["material_blend"]), {}),
    "set_light_shapes": ({}, lambda x: dict(x, light_shapes=cone_on_the_rect(x)), lambda c, y: c.set_light_shapes(y["light_shapes"]), {}),
    "set_light_shapes_removed": ({}, lambda x: without(x, "light_shapes"), lambda c, y: c.set_light_shapes(None), {}),
    "rebuild_option": ({}, lambda x: x, lambda c, y: c.set_option("bake_world", 0), {"bake_world": 0}),
    "update_accel_instances": ({}, lambda x: build(emit_xf=EMIT_XF_MOVED).arrays(), lambda c, y: c.update_accel(y["instances"]), {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_a_changed_input_renders_as_a_fresh_context(name):
    x_args, make_y, change, options = CASES[name]
    sc = build(**x_args)
    cam, x = sc.getCamera(), sc.arrays()
    y = make_y(x)
    n = len(x["instances"])
    c = make_ctx(x)
    f = None
    try:
        first = render(c, cam)
        before = derived(c, n)  # (every *_ensure has run: nothing is stale when the change arrives)
        change(c, y)
        if name == "update_accel_instances":
            assert c.build_info()["refit"] == 2  # (in place: the row is the update's own, not skh_set_instances')
        got = render(c, cam)
        got_derived = derived(c, n)
        f = make_ctx(y, options)
        want = render(f, cam)
        want_derived = derived(f, n)
    finally:
        c.close()
        if f is not None:
            f.close()
    assert np.array_equal(got, want), int((got != want).sum())
    assert got_derived == want_derived
    assert not np.array_equal(first, want) or before != want_derived  # (the change is one: X and Y differ in the image or in what is derived)


def test_setters_the_hierarchy_does_not_depend_on_cost_no_rebuild():
    """lights, materials, emission and the four per-material / per-light tables leave the in-place path open: observed as
    test_gpu_abi_misc.py::test_only_the_options_a_hierarchy_depends_on_cost_a_rebuild observes it, build_info().refit after skh_update_accel (2 in place, 0 a build)"""
    sc = build()
    x = sc.arrays()
    nm = len(x["materials"])
    mtex = np.zeros(nm, S.MATERIAL_TEXTURES)
    mtex["emission_channel"], mtex["roughness_scale"], mtex["metallic_scale"] = S.EMISSION_RGB, 1.0, 1.0
    mtex[2]["roughness_texture"] = 1
    setters = [("set_lights", lambda c: c.set_lights(x["lights"][::-1].copy())), ("set_materials", lambda c: c.set_materials(x["materials"])),
               ("set_emission", lambda c: c.set_emission(floor_emits(x))), ("set_material_textures", lambda c: c.set_material_textures(mtex)),
               ("set_material_cutouts", lambda c: c.set_material_cutouts(cutref.table(nm, {}))),
               ("set_material_blend", lambda c: c.set_material_blend(blendref.table(nm, {2: blendref.constant(0.5)}))),
               ("set_light_shapes", lambda c: c.set_light_shapes(cone_on_the_rect(x)))]
    c = make_ctx(x)
    try:
        c.update_accel(None)
        assert c.build_info()["refit"] == 2
        for name, call in setters:
            call(c)
            c.update_accel(None)
            assert c.build_info()["refit"] == 2, name
        c.set_option("bake_world", 4)  # (the control: its own value again, and the hierarchy is built anew)
        c.update_accel(None)
        assert c.build_info()["refit"] == 0
    finally:
        c.close()
