"""Fractional opacity on the GPU ("Fractional opacity"): skh_set_material_blend and the BLEND build of the k_cutout stage.

The yardsticks: tests/blendref.py (the draw in integer arithmetic, the transmittance's roundings) and, at the end points a = 0 and a = 1, the TWIN of
tests/test_gpu_cutout.py: the scene with the a = 0 triangles deleted, or the scene without a table.  Image comparisons are array_equal unless a bar is written
out.  Every test here fails without the feature: the entry points do not exist."""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import blendref, cutref
from tests.test_gpu_cutout import COUNTS, LAUNCHES, hits_equal, images_equal, make_ctx, render, with_emitter, with_environment

pytestmark = pytest.mark.gpu

F = np.float32
ZERO, FULL = np.zeros((4, 4), np.uint8), np.full((4, 4), 255, np.uint8)


def load(c, sc, blend=None, cut=None):
    arr = sc.arrays()
    c.set_scene(arr)
    c.set_material_cutouts(cut)
    c.set_material_blend(blend)
    return arr


def blend_of(cut):
    """the blend table that looks up what the cutout table `cut` looks up: active where that one has a threshold"""
    if cut is None:
        return None
    t = np.zeros(len(cut), S.MATERIAL_BLEND)
    for f in ("opacity_texture", "opacity_channel", "opacity_scale", "opacity_bias"):
        t[f] = cut[f]
    t["active"] = (cut["threshold"] > 0).astype(np.uint32)
    return t


def frame(c, sc, w, h, sample=0, spp=1, depth=1, accumulate=0):
    """one sub-frame of one sample, accumulation off: -> the output image's rgb"""
    import torch

    c.resize(w, h)
    img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    c.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=sample, spp_total=spp, max_depth=depth, enable_accumulation=accumulate), img.data_ptr())
    return img.cpu().numpy()[..., :3].copy()


def pixels(w, h):
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    return px.reshape(-1), py.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1: the probe
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_probe_equals_the_reference():
    rs = np.random.RandomState(3)
    n = 600
    t = np.stack([rs.randint(0, 4096, n), rs.randint(0, 4096, n), rs.randint(0, 1 << 16, n), rs.choice([1, 4, 64, 1024, 65536], n), rs.randint(0, 9, n),
                  rs.randint(0, 33, n)], -1).astype(np.uint32)
    t[0] = (4095, 4095, 65535, 65536, 8, 32)
    t[1] = 0
    t[2] = (0, 4095, 0, 1, 0, 32)
    c = make_ctx()
    got = c.blend_probe(t)
    want = blendref.xi(*[t[:, k] for k in range(6)])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got >= 0).all() and (got < 1).all() and len(np.unique(got)) > n - 5
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2: the end points, exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def bias_scene(twin, layout="single", extra=None, light=True):
    """the twin's card (the kept triangles, opaque) and, unless `twin`, the other triangles as a second mesh of a material of its own whose blend entry is the
    constant a = 0 -> (scene, blend table or None)"""
    def more(sc):
        mat = sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6))
        if extra is not None:
            extra(sc)
        if not twin:
            mesh = cutref.card_mesh(sc, ~cutref.card_kept(cutref.block_alpha()))
            for xf in cutref.CARD_XFORMS[layout]:
                sc.createInstance(S.INSTANCE_MESH, mesh, mat, xf)  # (behind every other mesh instance: their ids are the twin's)
        assert mat == 2

    sc, _, _ = cutref.card_scene(True, layout, extra=more, light=light)
    return sc, (None if twin else blendref.table(3, {2: blendref.constant(0.0)}))


@pytest.mark.parametrize("how", ["texture", "bias"])
@pytest.mark.parametrize("bake", [None, 0])
def test_zero_opacity_hit_records_equal_twin(how, bake):
    opts = {} if bake is None else {"bake_world": bake}
    layout = "shared" if bake == 0 else "single"
    if how == "texture":
        sc, cut, kept = cutref.card_scene(False, layout)
        tab = blend_of(cut)
    else:
        sc, tab = bias_scene(False, layout)
        kept = None
    tw = cutref.card_scene(True, layout)[0] if how == "texture" else bias_scene(True, layout)[0]
    cm, ct = make_ctx(**opts), make_ctx(**opts)
    arr = load(cm, sc, tab)
    load(ct, tw)
    cards = cutref.card_instances(arr)[:len(cutref.CARD_XFORMS[layout])]
    info = cm.blend_info()
    assert info["active_materials"] == 1 and info["instances"] == len(cutref.CARD_XFORMS[layout]) and ct.blend_info()["instances"] == 0
    for oblique in (False, True):
        for n in COUNTS:
            rays = cutref.card_rays(layout, oblique, n)
            cm.reset_stats()
            got, want = cm.trace(rays, 0), ct.trace(rays, 0)
            hits_equal(got, want, kept, cards if kept is not None else ())
            sh = cutref.shadow_version(rays)
            gs, ws = cm.trace(sh, 1), ct.trace(sh, 1)
            assert np.array_equal(gs["t"], ws["t"]) and set(np.unique(gs["t"])) <= {-1.0, 1.0}
            info = cm.blend_info()
            assert info["accepted_by_cap"] == 0
            if n >= 63:
                assert 0 < info["passed_radiance"] < n and info["crossed_shadow"] > 0 and (gs["t"] == 1).any() and (gs["t"] == -1).any()
    cm.close(), ct.close()


END_IMAGES = [("rect", "texture", {}), ("env", "texture", {}), ("emit", "texture", {}), ("rect", "bias", {}), ("env", "bias", {}), ("emit", "bias", {"bake_world": 0})]


@pytest.mark.parametrize("light,how,options", END_IMAGES, ids=["%s-%s-%d" % (c[0], c[1], len(c[2])) for c in END_IMAGES])
def test_zero_opacity_images_equal_twin(light, how, options):
    extra = {"rect": None, "env": with_environment, "emit": with_emitter}[light]
    if how == "texture":
        sc, cut, _ = cutref.card_scene(False, "single", extra=extra, light=light != "env")
        tab = blend_of(cut)
        tw = cutref.card_scene(True, "single", extra=extra, light=light != "env")[0]
    else:
        sc, tab = bias_scene(False, "single", extra, light != "env")
        tw = bias_scene(True, "single", extra, light != "env")[0]
    cm, ct = make_ctx(**options), make_ctx(**options)
    load(cm, sc, tab)
    load(ct, tw)
    a, b = render(cm, sc), render(ct, tw)
    images_equal(a, b)
    info = cm.blend_info()
    assert info["passed_radiance"] > 0 and info["crossed_shadow"] > 0 and info["accepted_by_cap"] == 0 and info["bytes"] > 0
    assert (a[3][..., :3] > 0).any() and ct.blend_info()["bytes"] == 0
    cm.set_material_blend(None)
    assert not np.array_equal(render(cm, sc)[3], a[3])  # (without the table the a = 0 triangles are there)
    cm.close(), ct.close()


@pytest.mark.parametrize("bake", [None, 0])
def test_full_opacity_equals_no_table(bake):
    opts = {} if bake is None else {"bake_world": bake}
    sc, _, _ = cutref.card_scene(False, "single")
    ones = blendref.table(2, {1: blendref.constant(1.0)})
    full = blend_of(cutref.card_scene(False, "single", alpha=FULL)[1])
    scf = cutref.card_scene(False, "single", alpha=FULL)[0]
    ca, cb = make_ctx(**opts), make_ctx(**opts)
    for scene, tab in ((sc, ones), (scf, full)):  # a constant 1; a texture that is 255 everywhere
        load(ca, scene, tab)
        load(cb, scene)
        assert ca.blend_info()["instances"] == 1
        ca.reset_stats()
        images_equal(render(ca, scene), render(cb, scene))
        for n in COUNTS:
            rays = cutref.card_rays("single", n % 2 == 1, n)
            assert ca.trace(rays, 0).tobytes() == cb.trace(rays, 0).tobytes()
            sh = cutref.shadow_version(rays)
            assert np.array_equal(ca.trace(sh, 1)["t"], cb.trace(sh, 1)["t"])
        info = ca.blend_info()
        assert info["passed_radiance"] == 0 and info["crossed_shadow"] == 0 and info["accepted_by_cap"] == 0
    ca.close(), cb.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3: the pass mask, exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
ENV_L = (0.5, 0.25, 2.0)


def wall_quad(sc, z, half=20.0, uv=None):
    return cutref.quad_mesh(sc, [(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)], uv)


def mask_scene(cards):
    """black diffuse cards (material 1) that fill the view of a camera on +Z, a constant environment behind them, nothing else"""
    sc = S.Scene()
    sc.addMaterial(S.MAT_DIFFUSE, (0.5, 0.5, 0.5))
    sc.addMaterial(S.MAT_DIFFUSE, (0.0, 0.0, 0.0))
    for k in range(cards):
        sc.createInstance(S.INSTANCE_MESH, wall_quad(sc, -1.0 * k), 1, np.eye(4))
    if cards == 0:
        sc.createInstance(S.INSTANCE_MESH, wall_quad(sc, 50.0, 0.5), 0, np.eye(4))  # (behind the camera: a scene needs a mesh)
    sc.setEnvironment(np.broadcast_to(np.float32(ENV_L), (4, 8, 3)).copy())
    sc.addCamera(cutref.camera((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 40.0))
    return sc


@pytest.mark.parametrize("cards", [1, 2])
def test_pass_mask_is_the_reference(cards):
    w, h, spp = 64, 48, 4
    bare = mask_scene(0)
    cb = make_ctx()
    load(cb, bare)
    env = frame(cb, bare, w, h)  # L as the miss program evaluates it, pixel by pixel
    assert (env > 0).all() and np.allclose(env, np.float32(ENV_L), rtol=1e-5)
    cb.close()
    sc = mask_scene(cards)
    c = make_ctx()
    load(c, sc)
    px, py = pixels(w, h)
    for a in (0.25, 0.5):
        c.set_material_blend(blendref.table(2, {1: blendref.constant(a)}))
        assert c.blend_info()["instances"] == cards
        for sample in range(4):
            c.reset_stats()
            img = frame(c, sc, w, h, sample, spp, depth=1)
            passed = np.ones(w * h, bool)
            for r in range(cards):
                passed &= ~blendref.accepts(a, px, py, sample, spp, 0, r)
            want = np.where(passed.reshape(h, w, 1), env, F(0.0)).astype(F)
            assert np.array_equal(img, want), (a, sample, int((img != want).any(-1).sum()))
            assert 0 < passed.sum() < w * h
            first = int((~blendref.accepts(a, px, py, sample, spp, 0, 0)).sum())
            assert c.blend_info()["passed_radiance"] == first + (int(passed.sum()) if cards == 2 else 0)
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4: shadow transmittance
# ---------------------------------------------------------------------------------------------------------------------------------------------
def shadow_scene(layers):
    """a diffuse floor under a distant light that shines straight down; black cards (material 1 + k for layer k) above the floor that shadow all
    of it and that the camera, which looks at the floor from below their height, does not see.
    The light's half-angle is 2 degrees, not 0: a cone of half-angle 0 has the pdf 1 / (2 pi (1 - cos 0)) = inf in this renderer (and in the reference's
    Lights.h), its sample weighs 0 and the image is black with or without a card -- which would compare 0 with 0.  The direction sampled in the cone comes from the
    path's sampler alone, so it is the same with and without the cards, and the cards (6 x 6 over a 4 x 4 floor, 1.5 above it) shadow all of the floor for
    every direction of the cone: each pixel's light sample is the same contribution in every scene of this test, crossed or not."""
    sc = S.Scene()
    sc.addMaterial(S.MAT_DIFFUSE, (0.7, 0.6, 0.5))
    for k in range(3):
        sc.addMaterial(S.MAT_DIFFUSE, (0.0, 0.0, 0.0))
    sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)]), 0, np.eye(4))
    for k in range(layers):
        y = 1.5 + 0.25 * k
        sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-3, y, 3), (3, y, 3), (3, y, -3), (-3, y, -3)]), 1 + k, np.eye(4))
    sc.createLight({"type": 3, "xform": S.rotate((1, 0, 0), math.radians(-90)), "useXform": True, "halfAngle": math.radians(2.0), "color": (1.0, 0.9, 0.8), "intensity": 3.0})
    sc.addCamera(cutref.camera((0.0, 0.6, 2.5), (0.0, 0.0, 0.0), 30.0))
    return sc


def test_shadow_transmittance():
    w, h = 48, 32
    c = make_ctx()
    plain = shadow_scene(0)
    load(c, plain)
    lit = frame(c, plain, w, h, accumulate=1)
    on = (lit > 0).all(-1)
    assert on.sum() > w * h // 3
    one, two = shadow_scene(1), shadow_scene(2)
    const = lambda *a: blendref.table(4, {1 + k: blendref.constant(v) for k, v in enumerate(a)})
    # powers of two: exact
    for scene, tab, factor in ((one, const(0.5), 0.5), (one, const(0.75), 0.25), (two, const(0.5, 0.5), 0.25), (one, const(0.0), 1.0), (two, const(0.0, 0.5), 0.5)):
        load(c, scene, tab)
        c.reset_stats()
        img = frame(c, scene, w, h)
        assert np.array_equal(img, (lit * F(factor)).astype(F)), factor
        info = c.blend_info()
        assert info["crossed_shadow"] == int(on.sum()) * len(scene.arrays()["instances"][1:-1]) and info["passed_radiance"] == 0
    # a = 0.3: the definition's roundings.  With u = 2^-24: w = fl(1 - a) = (1 - a)(1 + d0), |d0| <= u; per layer and channel one product, (1 + d), |d| <= u.
    # One layer: |got - c (1 - a)| <= c (1 - a) ((1 + u)^2 - 1); two layers: ((1 + u)^4 - 1).  a is the float32 the table holds; the sum 0 + c and the
    # accumulation of one sample are exact.
    u, a = 2.0 ** -24, float(F(0.3))
    for scene, tab, n in ((one, const(0.3), 1), (two, const(0.3, 0.3), 2)):
        load(c, scene, tab)
        img = frame(c, scene, w, h).astype(np.float64)
        want = lit.astype(np.float64) * (1.0 - a) ** n
        err = np.abs(img - want)
        bar = want * ((1.0 + u) ** (2 * n) - 1.0)
        print("a = 0.3, %d layer(s): largest error / bar = %.3f" % (n, float((err[on] / bar[on]).max())))
        assert (err <= bar).all() and (img[on] > 0).all()
        assert np.array_equal(img.astype(F), blendref.transmit(lit, [a] * n))  # (and the definition's own sequence of operations, bit for bit)
    # an opaque card behind a blended one; a blended one with a = 1
    load(c, two, const(0.5))
    assert (frame(c, two, w, h) == 0).all()
    load(c, two, const(0.5, 1.0))
    assert (frame(c, two, w, h) == 0).all()
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5: texture plateaus
# ---------------------------------------------------------------------------------------------------------------------------------------------
PLATEAUS = (0, 64, 128, 255)


def test_texture_plateaus():
    w, h = 64, 64
    tex = np.zeros((4, 32, 4), np.uint8)
    tex[..., :3] = 90
    for k, v in enumerate(PLATEAUS):
        tex[:, 8 * k:8 * k + 8, 3] = v
    sc = S.Scene()
    t = sc.addTexture(tex)
    sc.addMaterial(S.MAT_DIFFUSE, (0.5, 0.5, 0.5))
    sc.addMaterial(S.MAT_DIFFUSE, (0.0, 0.0, 0.0))
    # a quad over x, y in -1..1 at z = 0 with u = (x + 1) / 2: the camera (on +Z, fov 30 degrees at distance 3) sees x in -0.80..0.80
    sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], [(0, 0), (1, 0), (1, 1), (0, 1)]), 1, np.eye(4))
    sc.setEnvironment(np.broadcast_to(np.float32(ENV_L), (4, 8, 3)).copy())
    sc.addCamera(cutref.camera((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 30.0))
    c = make_ctx()
    load(c, sc, blendref.table(2, {1: blendref.entry(opacity_texture=t, opacity_channel=3)}))
    passed = np.stack([(frame(c, sc, w, h, s, 4) > 0).all(-1) for s in range(4)])  # 4 samples per pixel
    x = ((np.arange(w) + 0.5) / w * 2.0 - 1.0) * math.tan(math.radians(15.0)) * 3.0
    uu = (x + 1.0) / 2.0
    seen = 0
    for k, v in enumerate(PLATEAUS):
        cols = np.flatnonzero((uu > k / 4.0 + 2.5 / 32.0) & (uu < (k + 1) / 4.0 - 2.5 / 32.0))  # at least 2.5 texels from the plateau's borders
        assert len(cols) >= 6, (k, len(cols))
        blk = passed[:, 8:56, cols]
        n, p = blk.size, 1.0 - v / 255.0
        print("plateau %d: passed %d of %d, expected %.1f" % (v, int(blk.sum()), n, n * p))
        if v == 0:
            assert blk.all()
        elif v == 255:
            assert not blk.any()
        else:
            assert abs(int(blk.sum()) - n * p) <= 6.0 * math.sqrt(n * p * (1.0 - p))
        seen += 1
    assert seen == 4
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6: scheduling independence
# ---------------------------------------------------------------------------------------------------------------------------------------------
def busy_scene():
    """a room (identity transforms: a top level gives the bits of the baked world) under a tilted distant light and an environment, two blended cards above the
    floor that the camera sees and that the light's and the environment's shadow rays cross"""
    sc = S.Scene()
    sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    sc.addMaterial(S.MAT_DIFFUSE, (0.7, 0.3, 0.2))
    sc.addMaterial(S.MAT_DIFFUSE, (0.2, 0.4, 0.7))
    cutref.room(sc, 0, light=False)
    sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-0.9, 1.0, 0.9), (0.9, 1.0, 0.9), (0.9, 1.0, -0.9), (-0.9, 1.0, -0.9)]), 1, np.eye(4))
    sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-0.5, 1.4, 0.6), (0.7, 1.4, 0.6), (0.7, 1.4, -0.6), (-0.5, 1.4, -0.6)]), 2, np.eye(4))
    sc.createLight({"type": 3, "xform": S.rotate((1, 0, 0), math.radians(-70)), "useXform": True, "halfAngle": math.radians(4.0), "color": (1.0, 0.95, 0.9), "intensity": 4.0})
    with_environment(sc)
    sc.addCamera(cutref.camera())
    return sc, blendref.table(3, {1: blendref.constant(0.5), 2: blendref.constant(0.3)})


SCHEDULES = [({"compact_hits": 0}, {}), ({"compact_hits": 1}, {}), ({"overlap": 0}, {}), ({"overlap": 2}, {}), ({"subframe_batch": 0}, {}), ({"subframe_batch": 2}, {}),
             ({"subframe_batch": 3}, {}), ({"speculate": 0}, {"loop": True}), ({"speculate": 8}, {"loop": True}), ({"count_traversal": 1}, {}), ({"bake_world": 0}, {}),
             ({"bake_world": 0, "overlap": 2}, {"loop": True})]


def test_scheduling_independence():
    from strelka_amd import tiles

    sc, tab = busy_scene()
    w, h, how = 48, 48, {"spp": 6, "depth": 4}
    c = make_ctx()
    load(c, sc, tab)
    c.reset_stats()
    base = render(c, sc, w, h, **how)
    info = c.blend_info()
    assert info["passed_radiance"] > 0 and info["crossed_shadow"] > 0 and (base[0][..., :3] > 0).any()
    # tile subsets: two "ranks", each against its pixels of the full frame
    T = 16
    for rank in range(2):
        txy = tiles.assign_tiles(w, h, T, 2, rank)
        c.set_tiles(T, txy)
        part = render(c, sc, w, h, **how)[0]
        for (x0, y0) in np.asarray(txy).reshape(-1, 2):
            assert np.array_equal(part[y0:y0 + T, x0:x0 + T], base[0][y0:y0 + T, x0:x0 + T]), (rank, x0, y0)
    c.close()
    for options, extra in SCHEDULES:
        c = make_ctx(**options)
        load(c, sc, tab)
        got = render(c, sc, w, h, **dict(how, **extra))
        assert np.array_equal(got[0], base[0]), (options, extra, int((got[0] != base[0]).any(-1).sum()))
        c.close()
    # ... and the blend does something
    c = make_ctx()
    load(c, sc)
    assert not np.array_equal(render(c, sc, w, h, **how)[0], base[0])
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7: the round limit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_round_limit():
    eye = ((0.2, 3.4, 1.2), (0.0, 0.0, 0.0))
    layers = cutref.CARD_XFORMS["layers"]
    sc, cut, _ = cutref.card_scene(False, "layers", alpha=ZERO, eye=eye)
    tab = blend_of(cut)
    bare, _, _ = cutref.card_scene(False, "layers", alpha=ZERO, eye=eye, cards=False)
    third, _, _ = cutref.card_scene(False, "layers", alpha=FULL, eye=eye, xforms=layers[:1])  # the lowest layer alone, opaque: what a ray from above meets third
    cm, cb, c3 = make_ctx(), make_ctx(), make_ctx()
    arr = load(cm, sc, tab)
    load(cb, bare)
    load(c3, third)
    rays = cutref.card_rays("layers", False, 4096)
    sh = np.array(rays, copy=True)
    sh["tmax"] = np.where(np.arange(len(sh)) % 2 == 0, 2.4, 6.0).astype(np.float32)  # ends between the lowest layer and the floor | reaches the floor
    # cutout_rounds 8 (the default): the cards are not there
    cm.reset_stats()
    hits_equal(cm.trace(rays, 0), cb.trace(rays, 0))
    assert cm.blend_info()["passed_radiance"] == 3 * len(rays)
    gs = cm.trace(sh, 1)
    assert np.array_equal(gs["t"], cb.trace(sh, 1)["t"]) and (gs["t"] == -1).sum() == len(sh) // 2
    info = cm.blend_info()
    assert info["crossed_shadow"] == 3 * len(rays) and info["accepted_by_cap"] == 0
    images_equal(render(cm, sc), render(cb, bare))
    # 2: two hits passed, then the third card is accepted whatever its opacity -- and occludes a shadow ray
    cm.set_option("cutout_rounds", 2)
    cm.reset_stats()
    got, want = cm.trace(rays, 0), c3.trace(rays, 0)
    lowest = cutref.card_instances(arr)[0]
    assert (want["instance_id"] == lowest).all()
    hits_equal(got, want)
    info = cm.blend_info()
    assert info["passed_radiance"] == 2 * len(rays) and info["accepted_by_cap"] == len(rays)
    gs = cm.trace(sh, 1)
    assert np.array_equal(gs["t"], c3.trace(sh, 1)["t"]) and (gs["t"] == 1).all()
    assert cm.blend_info()["accepted_by_cap"] == 2 * len(rays) and cm.cutout_info()["accepted_by_cap"] == 0
    # in a frame: a camera above the three layers sees the lowest one, opaque, where the twin has it; its shadow rays are occluded by a card above them
    img = render(cm, sc, depth=1)[0]
    assert np.isfinite(img).all()
    # 1: the second card
    cm.set_option("cutout_rounds", 1)
    got = cm.trace(rays, 0)
    assert (got["instance_id"] == lowest + 1).all() and np.allclose(got["t"], 1.8, atol=1e-5)
    for c in (cm, cb, c3):
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8: cutouts and blending along one ray; curves beside a blended card
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend_first", [False, True])
def test_cutout_and_blend_along_one_ray(blend_first):
    layers = cutref.CARD_XFORMS["layers"]
    lo, hi = layers[0], layers[2]  # (a ray from above meets `hi` first)

    def more(sc):
        mat = sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6))
        assert mat == 2
        sc.createInstance(S.INSTANCE_MESH, cutref.card_mesh(sc), mat, hi if blend_first else lo)

    sc, cut, _ = cutref.card_scene(False, "layers", alpha=ZERO, xforms=[lo if blend_first else hi], extra=more)  # material 1: the cutout, wholly cut
    bare, _, _ = cutref.card_scene(False, "layers", alpha=ZERO, cards=False)
    cm, cb = make_ctx(), make_ctx()
    load(cm, sc, blendref.table(3, {2: blendref.constant(0.0)}), cut)
    load(cb, bare)
    rays = cutref.card_rays("layers", False, 4096)
    cm.reset_stats()
    hits_equal(cm.trace(rays, 0), cb.trace(rays, 0))
    sh = np.array(rays, copy=True)
    sh["tmax"] = np.where(np.arange(len(sh)) % 2 == 0, 2.4, 6.0).astype(np.float32)  # ends between the lower card and the floor | reaches the floor
    assert np.array_equal(cm.trace(sh, 1)["t"], cb.trace(sh, 1)["t"])
    bi, ci = cm.blend_info(), cm.cutout_info()
    assert bi["passed_radiance"] == len(rays) and ci["continued_closest"] == len(rays) and bi["crossed_shadow"] == len(rays) and ci["continued_shadow"] == len(rays)
    images_equal(render(cm, sc), render(cb, bare))
    # every passed hit uses up a round: with one round the second card is accepted whatever it is
    cm.set_option("cutout_rounds", 1)
    cm.reset_stats()
    got = cm.trace(rays, 0)
    assert np.isin(got["instance_id"], cutref.card_instances(sc.arrays())).all()
    assert cm.blend_info()["accepted_by_cap"] + cm.cutout_info()["accepted_by_cap"] == len(rays)
    cm.close(), cb.close()


def test_curves_beside_a_blended_card():
    from tests.test_gpu_cutout import groom_scene

    sc, cut, kept, ids = groom_scene(False)
    tw, _, _, _ = groom_scene(True)
    cm, ct = make_ctx(), make_ctx()
    arr = load(cm, sc, blend_of(cut))
    load(ct, tw)
    curve = [k for k, i in enumerate(arr["instances"]) if int(i["type"]) == S.INSTANCE_CURVE]
    rays = cutref.card_rays("front", False, 4096)
    hits_equal(cm.trace(rays, 0), ct.trace(rays, 0), kept, ids)
    # a blend entry on the curves' own material changes nothing: curves are never blended
    hair_mat = int(arr["instances"][curve[0]]["material_id"])
    t = blend_of(cut)
    t[hair_mat] = blendref.constant(0.0)
    rs = np.random.RandomState(12)
    d = rs.normal(size=(2048, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = -np.abs(d[:, 2])
    org = d * 3.0 + np.array([0.0, 0.0, 0.4])
    tg = rs.normal(size=(2048, 3))
    tg = tg / np.linalg.norm(tg, axis=1, keepdims=True) * rs.uniform(1.0, 1.4, (2048, 1))
    hair = cutref.make_rays(org, tg)
    a = cm.trace(hair, 0)
    uses = [k for k, i in enumerate(arr["instances"]) if int(i["type"]) == S.INSTANCE_MESH and int(i["material_id"]) == hair_mat]
    if not uses and hair_mat < len(t):  # (a mesh of the hair's material would be blended: only then is the comparison about curves)
        cm.set_material_blend(t)
        assert cm.trace(hair, 0).tobytes() == a.tobytes()
    assert (a["instance_id"] == curve[0]).sum() > 10
    cm.set_material_blend(blend_of(cut))
    images_equal(render(cm, sc, 32, 32), render(ct, tw, 32, 32))
    assert cm.blend_info()["passed_radiance"] > 0
    cm.close(), ct.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 9: additivity
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_additivity():
    sc, cut, _ = cutref.card_scene(False, "single")
    sc.addMaterial(S.MAT_DIFFUSE, (0.3, 0.3, 0.3))  # material 2: nobody uses it
    tab = blendref.table(3, {1: blendref.constant(0.5)})
    never, removed, inactive, unused = make_ctx(), make_ctx(), make_ctx(), make_ctx()
    load(never, sc)
    load(removed, sc, tab)
    render(removed, sc)  # (the stage has run and its buffers exist)
    assert removed.blend_info()["bytes"] > 0 and removed.cutout_info()["bytes"] > 0
    removed.set_material_blend(None)
    off = np.array(tab, copy=True)
    off["active"] = 0
    load(inactive, sc, off)
    load(unused, sc, blendref.table(3, {2: blendref.constant(0.5)}))
    out = []
    for c in (never, removed, inactive, unused):
        c.reset_stats()
        img = render(c, sc)
        st = c.stats()
        out.append((img, [st[k] for k in LAUNCHES], st["rays_radiance"], st["rays_shadow"]))
        info = c.blend_info()
        assert info["instances"] == 0 and info["passed_radiance"] == 0 and info["crossed_shadow"] == 0 and info["bytes"] == 0 and c.cutout_info()["bytes"] == 0
    assert unused.blend_info()["active_materials"] == 1
    for img, launches, rr, rsh in out[1:]:
        images_equal(img, out[0][0])
        assert launches == out[0][1] and (rr, rsh) == out[0][2:]
    # threshold cutouts alone: an unused blend table beside them changes nothing
    load(never, sc, None, cut)
    want = render(never, sc)
    never.reset_stats()
    render(never, sc)
    la = [never.stats()[k] for k in LAUNCHES]
    never.set_material_blend(blendref.table(3, {2: blendref.constant(0.5)}))
    never.reset_stats()
    images_equal(render(never, sc), want)
    assert [never.stats()[k] for k in LAUNCHES] == la and never.blend_info()["instances"] == 0 and never.cutout_info()["instances"] == 1
    for c in (never, removed, inactive, unused):
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 10: staleness
# ---------------------------------------------------------------------------------------------------------------------------------------------
def snapshot(c, sc):
    rays = cutref.card_rays("single", False, 1024)
    return c.trace(rays, 0).tobytes(), c.trace(cutref.shadow_version(rays), 1)["t"].tobytes(), render(c, sc, 32, 32)


def same_snapshot(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    images_equal(a[2], b[2])


def fresh(sc, tab, arr=None):
    c = make_ctx()
    if arr is None:
        load(c, sc, tab)
    else:
        c.set_scene(arr)
        c.set_material_blend(tab)
    s = snapshot(c, sc)
    c.close()
    return s


def soft(tab):
    """the plateau table with a fractional end: a = 0.5 * alpha -- the kept triangles are gambled on, the others passed"""
    t = np.array(tab, copy=True)
    t["opacity_scale"] = np.where(t["active"] != 0, 0.5, t["opacity_scale"])
    return t


def test_staleness():
    sc, cut, _ = cutref.card_scene(False, "single")
    tab = soft(blend_of(cut))
    c = make_ctx()
    arr = load(c, sc, tab)
    first = snapshot(c, sc)
    # new textures: the alpha pattern swapped
    flipped, fcut, _ = cutref.card_scene(False, "single", alpha=cutref.block_alpha(flip=True))
    c.set_textures(flipped.arrays()["textures"])
    s = snapshot(c, sc)
    same_snapshot(s, fresh(flipped, soft(blend_of(fcut))))
    assert s[0] != first[0]
    c.set_textures(arr["textures"])
    same_snapshot(snapshot(c, sc), first)
    # new materials: the blended material in another slot (the instances and the table follow it)
    moved, mcut, _ = cutref.card_scene(False, "single", cut_slot=2)
    mtab = soft(blend_of(mcut))
    marr = moved.arrays()
    c.set_materials(marr["materials"])
    c.set_instances(marr["instances"])
    c.set_material_blend(mtab)
    same_snapshot(snapshot(c, sc), first)
    assert c.blend_info()["instances"] == 1
    c.set_material_blend(tab)  # the old table on the new materials: slot 1 is a grey nobody uses
    assert c.blend_info()["instances"] == 0
    same_snapshot(snapshot(c, sc), fresh(moved, None))
    c.set_material_blend(mtab)
    # skh_update_accel with a new instance table: the card moved
    shift = S.translate((0.8, 0.0, -0.4))
    inst2 = np.array(marr["instances"], copy=True)
    card = cutref.card_instances(marr)[0]
    t = np.eye(4)
    t[:3, :] = np.asarray(inst2[card]["transform"], np.float64).reshape(3, 4)
    inst2[card]["transform"] = (shift @ t)[:3, :].astype(np.float32).reshape(12)
    c.update_accel(inst2)
    moved2, _, _ = cutref.card_scene(False, "single", cut_slot=2, xforms=[shift @ cutref.CARD_XFORMS["single"][0]])
    same_snapshot(snapshot(c, sc), fresh(moved2, mtab))
    # a refit after a vertex edit of the card: raised by 0.1
    arr3 = moved2.arrays()
    me = arr3["meshes"][int(arr3["instances"][card]["geom_id"])]
    v0, v1 = int(me["vertex_offset"]), int(me["vertex_offset"]) + int(me["vertex_count"])
    arr3["vertices"]["pos"][v0:v1, 1] += np.float32(0.1)
    c.set_geometry(arr3)
    c.refit_accel()
    same_snapshot(snapshot(c, sc), fresh(sc, mtab, arr3))
    assert c.blend_info()["instances"] == 1
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 11: refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from strelka_amd import capi

    sc, cut, _ = cutref.card_scene(False, "single")
    tab = soft(blend_of(cut))
    c = make_ctx()
    load(c, sc, tab)
    want = render(c, sc, 32, 32)
    bad = []
    for field, value in (("opacity_channel", 4), ("opacity_scale", np.nan), ("opacity_scale", np.inf), ("opacity_bias", -np.inf), ("active", 2)):
        t = np.array(tab, copy=True)
        t[field][1] = value
        bad.append((t, b"material 1"))
    for k in range(3):
        t = np.array(tab, copy=True)
        t["reserved"][1, k] = 7
        bad.append((t, b"material 1"))
    bad.append((blendref.table(3, {1: tab[1]}), b"3 entries for 2 materials"))  # more entries than materials
    for t, msg in bad:
        st = c.lib.skh_set_material_blend(c.h, t.ctypes.data_as(capi.C.c_void_p), len(t))
        assert st == 3, (st, t)  # SKH_INVALID_ARGUMENT
        err = c.lib.skh_last_error(c.h)
        assert b"skh_set_material_blend" in err and msg in err, err
        images_equal(render(c, sc, 32, 32), want)  # the previous table is still in effect
    assert c.blend_info()["instances"] == 1
    calls = (lambda: render(c, sc, 32, 32), lambda: c.trace(cutref.card_rays("single", False, 63), 0), lambda: c.blend_info())
    # a material that emits and is blended: refused by the call that would use it; gone with either of the two
    le = np.zeros((2, 3), np.float32)
    le[1] = (1.0, 2.0, 3.0)
    c.set_emission(le)
    for call in calls:
        with pytest.raises(capi.SkhError, match="material 1 both emits"):
            call()
    c.set_emission(None)
    images_equal(render(c, sc, 32, 32), want)
    # a material with a cutout and a blend entry
    c.set_material_cutouts(cut)
    for call in calls:
        with pytest.raises(capi.SkhError, match="material 1 has both"):
            call()
    c.set_material_cutouts(None)
    images_equal(render(c, sc, 32, 32), want)  # the table survived both
    # an emitter beside a blended material is fine
    le[0], le[1] = (0.5, 0.5, 0.5), 0.0
    c.set_emission(le)
    assert np.isfinite(render(c, sc, 32, 32)[0]).all()
    c.close()
