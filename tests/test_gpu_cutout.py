"""Cutouts on the GPU ("Cutouts"): skh_set_material_cutouts and the k_cutout stage between trace and shade.

The yardstick is the TWIN: a card of 32 triangles with unshared vertices whose three vertices carry one uv -- the centre of a 2 x 2-texel block of an 8 x 8
texture whose alpha is 0 or 255 per block -- is wholly kept or wholly cut triangle by triangle, so the masked scene must give, bit for bit, the hit records and
the images of the same scene with the cut triangles deleted.  Beside it tests/cutref.py: the definition as a loop over the CPU checker's closest-hit query.
All comparisons are array_equal.  Every test here fails without the feature: the setter does not exist."""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import cutref

pytestmark = pytest.mark.gpu

F = np.float32
NO_ID = 0xFFFFFFFF
COUNTS = (1, 63, 65, 4096)  # partial waves, empty shards, more than one block per shard
HIT_CASES = [(layout, oblique, n) for layout in ("single", "shared") for oblique in (False, True) for n in COUNTS] + [("layers", False, 4096), ("front", False, 4096)]


def make_ctx(**options):
    from strelka_amd import build, capi

    build.build()
    c = capi.Context(0)
    for k, v in options.items():
        c.set_option(k, v)
    return c


def load(c, sc, tab):
    arr = sc.arrays()
    c.set_scene(arr)
    c.set_material_cutouts(tab)
    return arr


def render(c, sc, w=48, h=48, spp=2, depth=3, loop=False, **kw):
    """-> the accumulator, both AOVs and the output image (debug views go there, not to the accumulator).  One call for all sub-frames (the batched pass),
    or `loop`: one sub-frame per call"""
    import torch

    c.resize(w, h)
    cam = sc.getCamera()
    img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    if loop:
        for i in range(spp):
            c.render_subframe(S.frame_params(cam, w, h, subframe_index=i, spp_total=spp, max_depth=depth, **kw), img.data_ptr())
    else:
        c.render_subframes(S.frame_params(cam, w, h, subframe_index=0, spp_total=spp, max_depth=depth, **kw), spp, img.data_ptr())
    return c.read_accum(), c.read_aov(0), c.read_aov(1), img.cpu().numpy()


def images_equal(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), int((x.view(np.uint32) != y.view(np.uint32)).sum())


def hits_equal(got, want, prim_map=None, cards=()):
    for f in ("t", "u", "v", "instance_id"):
        assert np.array_equal(got[f], want[f]), (f, int((got[f] != want[f]).sum()))
    prim = want["prim_id"]
    if prim_map is not None:
        on_card = np.isin(want["instance_id"], list(cards))
        prim = np.where(on_card, prim_map[np.minimum(prim, len(prim_map) - 1)], prim)
    assert np.array_equal(got["prim_id"], prim)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1: hit records, masked = twin = the reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,bake", [("single", None), ("single", 0), ("shared", None), ("shared", 0)])  # (shared, bake 0: the two-level kernel)
def test_hit_records_masked_equals_twin(layout, bake, ork):
    from tests import orklib

    opts = {} if bake is None else {"bake_world": bake}
    sc, tab, kept = cutref.card_scene(False, layout)
    tw, _, _ = cutref.card_scene(True, layout)
    cm, ct = make_ctx(**opts), make_ctx(**opts)
    arr = load(cm, sc, tab)
    load(ct, tw, None)
    cards = cutref.card_instances(arr)
    assert len(cards) == len(cutref.CARD_XFORMS[layout])
    info = cm.cutout_info()
    assert info["active_materials"] == 1 and info["instances"] == len(cards) and ct.cutout_info()["instances"] == 0
    o = orklib.new_context()
    o.set_bake(4 if bake is None else bake)
    o.set_scene(arr)
    cut_prims = np.setdiff1d(np.arange(32), kept)
    for _, oblique, n in [c for c in HIT_CASES if c[0] == layout]:
        rays = cutref.card_rays(layout, oblique, n)
        cm.reset_stats()
        got, want = cm.trace(rays, 0), ct.trace(rays, 0)
        hits_equal(got, want, kept, cards)
        # the rays continued are exactly those whose first hit is a cut triangle (a card lies in nobody's way to another card here)
        cm.set_material_cutouts(None)
        first = cm.trace(rays, 0)
        cm.set_material_cutouts(tab)
        n_cut = int((np.isin(first["instance_id"], cards) & np.isin(first["prim_id"], cut_prims)).sum())
        info = cm.cutout_info()
        assert info["continued_closest"] == n_cut and info["continued_shadow"] == 0 and info["accepted_by_cap"] == 0
        if n >= 63:
            assert 0 < n_cut < n
        sh = cutref.shadow_version(rays)
        gs, ws = cm.trace(sh, 1), ct.trace(sh, 1)
        assert np.array_equal(gs["t"], ws["t"]) and set(np.unique(gs["t"])) <= {-1.0, 1.0}
        if n >= 63:
            assert (gs["t"] == 1).any() and (gs["t"] == -1).any()
        if n <= 65 or not oblique:
            # ... and the reference's
            ref, rinfo = cutref.trace(o, arr, tab, rays, 0)
            assert got.tobytes() == ref.tobytes() and rinfo["continued"] == n_cut
            rs, _ = cutref.trace(o, arr, tab, sh, 1)
            assert np.array_equal(gs["t"], rs["t"])
    cm.close(), ct.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2: the interpolated uv against the reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bake", [None, 0])
def test_interpolated_uv_against_the_reference(bake, ork):
    from tests import orklib

    sc, tex = cutref.half_scene()
    c = make_ctx(**({} if bake is None else {"bake_world": bake}))
    arr = load(c, sc, None)
    o = orklib.new_context()
    o.set_bake(4 if bake is None else bake)
    o.set_scene(arr)
    rays, u = cutref.half_rays()
    left = u < 0.5
    plain = c.trace(rays, 0)
    quad = int(plain["instance_id"][0])
    assert (plain["instance_id"] == quad).all() and int(arr["instances"][quad]["material_id"]) == 1
    sh = np.array(rays, copy=True)
    sh["tmax"] = plain["t"] + F(0.3)  # ends between the quad and the floor
    cases = [(cutref.entry(opacity_texture=tex, opacity_channel=3, threshold=0.5), left),                                        # alpha: the left half is cut
             (cutref.entry(opacity_texture=tex, opacity_channel=0, opacity_scale=-1.0, opacity_bias=1.0, threshold=0.5), ~left),  # 1 - red: the decision inverted
             (cutref.entry(opacity_texture=tex, opacity_channel=3, threshold=1.0), left),                                        # 255 / 255 >= 1
             (cutref.entry(opacity_texture=tex, opacity_channel=3, threshold=1.0 / 255.0), left),                                # 0 < 1 / 255
             (cutref.entry(opacity_texture=tex + 5, opacity_channel=3, opacity_scale=0.25, opacity_bias=0.25, threshold=0.5), ~np.ones(len(u), bool)),  # no such texture: texel 1 -> 0.5
             (cutref.entry(opacity_scale=0.0, opacity_bias=0.25, threshold=0.5), np.ones(len(u), bool))]                         # a constant below the threshold
    for e, cut in cases:
        tab = cutref.table(2, {1: e})
        c.set_material_cutouts(tab)
        c.reset_stats()
        got = c.trace(rays, 0)
        assert np.array_equal(got["instance_id"] != quad, cut)
        assert c.cutout_info()["continued_closest"] == int(cut.sum())
        ref, _ = cutref.trace(o, arr, tab, rays, 0, margin=1.5)
        assert got.tobytes() == ref.tobytes()
        gs = c.trace(sh, 1)
        rs, _ = cutref.trace(o, arr, tab, sh, 1, margin=1.5)
        assert np.array_equal(gs["t"] == -1, cut) and np.array_equal(gs["t"], rs["t"])
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3: images, masked = twin
# ---------------------------------------------------------------------------------------------------------------------------------------------
def with_environment(sc):
    rs = np.random.RandomState(21)
    env = rs.uniform(0.05, 1.0, (4, 8, 3)).astype(np.float32)
    env[1, 2] = (40.0, 30.0, 20.0)
    sc.setEnvironment(env)


def with_emitter(sc):
    """an emissive quad under the ceiling that faces down, beside the rect light: the MIS hit path and the shortened shadow rays"""
    lamp = sc.addMaterial(S.MAT_DIFFUSE, (0.1, 0.1, 0.1), emission=(6.0, 5.0, 4.0))
    sc.createInstance(S.INSTANCE_MESH, cutref.quad_mesh(sc, [(-1.6, 2.6, -0.5), (-0.8, 2.6, -0.5), (-0.8, 2.6, 0.5), (-1.6, 2.6, 0.5)]), lamp, np.eye(4))


IMAGE_CASES = [("rect", {}, {}), ("env", {}, {}), ("emit", {}, {}), ("rect", {"bake_world": 0}, {}), ("emit", {"bake_world": 0}, {}),
               ("rect", {"compact_hits": 0}, {}), ("rect", {"compact_hits": 1}, {}), ("rect", {"overlap": 0}, {}), ("rect", {"overlap": 2}, {}),
               ("rect", {"subframe_batch": 0}, {}), ("rect", {"subframe_batch": 2}, {}), ("env", {"speculate": 8}, {"loop": True, "spp": 6}),
               ("rect", {"count_traversal": 1}, {}), ("rect", {}, {"debug": 1}), ("rect", {"bake_world": 0, "overlap": 2}, {"layout": "shared"})]


@pytest.mark.parametrize("light,options,how", IMAGE_CASES, ids=["%d-%s" % (k, "-".join([c[0]] + ["%s%s" % kv for d in c[1:] for kv in d.items()])) for k, c in enumerate(IMAGE_CASES)])
def test_images_masked_equals_twin(light, options, how):
    how = dict(how)
    layout = how.pop("layout", "single")
    extra = {"rect": None, "env": with_environment, "emit": with_emitter}[light]
    sc, tab, _ = cutref.card_scene(False, layout, extra=extra, light=light != "env")
    tw, _, _ = cutref.card_scene(True, layout, extra=extra, light=light != "env")
    cm, ct = make_ctx(**options), make_ctx(**options)
    load(cm, sc, tab)
    load(ct, tw, None)
    a, b = render(cm, sc, **how), render(ct, tw, **how)
    images_equal(a, b)
    info = cm.cutout_info()
    assert info["continued_closest"] > 0 and info["accepted_by_cap"] == 0 and info["bytes"] > 0
    if how.get("debug", 0) != 1:
        assert info["continued_shadow"] > 0
    assert (a[3][..., :3] > 0).any() and ct.cutout_info()["bytes"] == 0
    # the cutout does something: the same scene without the table renders another image
    cm.set_material_cutouts(None)
    assert not np.array_equal(render(cm, sc, **how)[3], a[3])
    cm.close(), ct.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4: layers and the round limit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_layers_and_the_round_limit():
    zero = np.zeros((4, 4), np.uint8)  # fully cut
    full = np.full((4, 4), 255, np.uint8)
    eye = ((0.2, 3.4, 1.2), (0.0, 0.0, 0.0))
    layers = cutref.CARD_XFORMS["layers"]
    sc, tab, _ = cutref.card_scene(False, "layers", alpha=zero, eye=eye)
    bare, _, _ = cutref.card_scene(False, "layers", alpha=zero, eye=eye, cards=False)
    third, _, _ = cutref.card_scene(False, "layers", alpha=full, eye=eye, xforms=layers[:1])  # the lowest layer alone, opaque: what a ray from above meets third
    cm, cb, c3 = make_ctx(), make_ctx(), make_ctx()
    arr = load(cm, sc, tab)
    load(cb, bare, None)
    load(c3, third, None)
    rays = cutref.card_rays("layers", False, 4096)
    sh = np.array(rays, copy=True)
    sh["tmax"] = np.where(np.arange(len(sh)) % 2 == 0, 2.4, 6.0).astype(np.float32)  # ends between the lowest layer and the floor | reaches the floor
    # the default round limit: the cards are not there; three rejections per ray, so no rejected primitive was ever hit again
    cm.reset_stats()
    hits_equal(cm.trace(rays, 0), cb.trace(rays, 0))
    assert cm.cutout_info()["continued_closest"] == 3 * len(rays)
    gs = cm.trace(sh, 1)
    assert np.array_equal(gs["t"], cb.trace(sh, 1)["t"]) and (gs["t"] == -1).sum() == len(sh) // 2
    info = cm.cutout_info()
    assert info["continued_shadow"] == 3 * len(rays) and info["accepted_by_cap"] == 0
    images_equal(render(cm, sc), render(cb, bare))
    # cutout_rounds 2: two rejections, then the third card is accepted whatever its opacity -- for closest and for shadow
    cm.set_option("cutout_rounds", 2)
    cm.reset_stats()
    got, want = cm.trace(rays, 0), c3.trace(rays, 0)
    lowest = cutref.card_instances(arr)[0]
    assert (want["instance_id"] == lowest).all()
    hits_equal(got, want)
    info = cm.cutout_info()
    assert info["continued_closest"] == 2 * len(rays) and info["accepted_by_cap"] == len(rays)
    gs = cm.trace(sh, 1)
    assert np.array_equal(gs["t"], c3.trace(sh, 1)["t"]) and (gs["t"] == 1).all()
    assert cm.cutout_info()["accepted_by_cap"] == 2 * len(rays)
    # ... and 1: the second one
    cm.set_option("cutout_rounds", 1)
    got = cm.trace(rays, 0)
    assert (got["instance_id"] == lowest + 1).all() and np.allclose(got["t"], 1.8, atol=1e-5)
    # the round limit renders, too (no bit-level twin: a path from below meets the layers in the other order)
    cm.set_option("cutout_rounds", 2)
    img = render(cm, sc)[0]
    assert np.isfinite(img).all() and (img[..., :3] > 0).any()
    for c in (cm, cb, c3):
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5: a round with nothing to do, a round with everything to do
# ---------------------------------------------------------------------------------------------------------------------------------------------
LAUNCHES = ("launches_trace_closest", "launches_trace_shadow", "launches_shade", "launches_other")


def test_unused_material_and_all_rays_continued():
    # a table whose only active material is used by no instance: the bits, the launches and the memory of no table
    sc, tab, _ = cutref.card_scene(False, "single", cut_slot=1)
    unused = cutref.table(3, {2: cutref.entry(opacity_scale=0.0, opacity_bias=0.0, threshold=0.5)})
    sc3, _, _ = cutref.card_scene(False, "single", cut_slot=1)
    sc3.addMaterial(S.MAT_DIFFUSE, (0.3, 0.3, 0.3))
    ca, cb = make_ctx(), make_ctx()
    load(ca, sc3, unused)
    load(cb, sc3, None)
    ca.reset_stats(), cb.reset_stats()
    images_equal(render(ca, sc3), render(cb, sc3))
    info = ca.cutout_info()
    assert info["active_materials"] == 1 and info["instances"] == 0 and info["bytes"] == 0 and info["continued_closest"] == 0
    sa, sb = ca.stats(), cb.stats()
    assert [sa[k] for k in LAUNCHES] == [sb[k] for k in LAUNCHES]
    ca.close(), cb.close()
    # a camera that sees only the (fully cut) card: every primary ray continues
    zero = np.zeros((4, 4), np.uint8)
    eye = ((0.0, 1.5, 0.0), (0.0, 0.0, 0.001), 60.0)  # half a unit above the card, looking down: the card fills the view
    sc, tab, _ = cutref.card_scene(False, "single", alpha=zero, eye=eye)
    bare, _, _ = cutref.card_scene(False, "single", alpha=zero, eye=eye, cards=False)
    cm, cb = make_ctx(), make_ctx()
    load(cm, sc, tab)
    load(cb, bare, None)
    cm.reset_stats()
    images_equal(render(cm, sc, spp=1, depth=1), render(cb, bare, spp=1, depth=1))
    assert cm.cutout_info()["continued_closest"] == 48 * 48
    cm.close(), cb.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6: additivity
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_additivity():
    sc, tab, _ = cutref.card_scene(False, "single")
    never, removed, zeros = make_ctx(), make_ctx(), make_ctx()
    load(never, sc, None)
    load(removed, sc, tab)
    render(removed, sc)  # (the cutout stage has run and its buffers exist)
    assert removed.cutout_info()["bytes"] > 0
    removed.set_material_cutouts(None)
    load(zeros, sc, cutref.table(2, {1: cutref.entry(opacity_texture=1, threshold=0.0)}))
    out = []
    for c in (never, removed, zeros):
        c.reset_stats()
        img = render(c, sc)
        st = c.stats()
        out.append((img, [st[k] for k in LAUNCHES], st["rays_radiance"], st["rays_shadow"]))
        info = c.cutout_info()
        assert info["instances"] == 0 and info["continued_closest"] == 0 and info["continued_shadow"] == 0 and info["bytes"] == 0
    for img, launches, rr, rsh in out[1:]:
        images_equal(img, out[0][0])
        assert launches == out[0][1] and (rr, rsh) == out[0][2:]
    assert out[0][1][1] > 0  # (any-hit launches were counted)
    # with the table the SAME rays are counted: continued rays are not rays_radiance / rays_shadow
    removed.set_material_cutouts(tab)
    tw, _, _ = cutref.card_scene(True, "single")
    ct = make_ctx()
    load(ct, tw, None)
    removed.reset_stats(), ct.reset_stats()
    images_equal(render(removed, sc), render(ct, tw))
    sa, sb = removed.stats(), ct.stats()
    assert (sa["rays_radiance"], sa["rays_shadow"]) == (sb["rays_radiance"], sb["rays_shadow"])
    for c in (never, removed, zeros, ct):
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7: staleness
# ---------------------------------------------------------------------------------------------------------------------------------------------
def snapshot(c, sc, layout="single"):
    rays = cutref.card_rays(layout, False, 1024)
    return c.trace(rays, 0).tobytes(), c.trace(cutref.shadow_version(rays), 1)["t"].tobytes(), render(c, sc, 32, 32)


def same_snapshot(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    images_equal(a[2], b[2])


def fresh(sc, tab):
    c = make_ctx()
    load(c, sc, tab)
    s = snapshot(c, sc)
    c.close()
    return s


def test_staleness():
    sc, tab, _ = cutref.card_scene(False, "single")
    c = make_ctx()
    arr = load(c, sc, tab)
    first = snapshot(c, sc)
    # skh_set_textures swapping the alpha pattern
    flipped, ftab, _ = cutref.card_scene(False, "single", alpha=cutref.block_alpha(flip=True))
    c.set_textures(flipped.arrays()["textures"])
    s = snapshot(c, sc)
    same_snapshot(s, fresh(flipped, ftab))
    assert s[0] != first[0]
    c.set_textures(arr["textures"])
    same_snapshot(snapshot(c, sc), first)
    # skh_set_materials moving the cutout material to another slot (the instances and the table follow it)
    moved, mtab, _ = cutref.card_scene(False, "single", cut_slot=2)
    marr = moved.arrays()
    c.set_materials(marr["materials"])
    c.set_instances(marr["instances"])
    c.set_material_cutouts(mtab)
    same_snapshot(snapshot(c, sc), first)  # (the same picture: grey is grey in every slot)
    assert c.cutout_info()["instances"] == 1
    # ... and the old table on the new materials: slot 1 is now a grey nobody uses -- no cutout in use, the card opaque
    c.set_material_cutouts(tab)
    assert c.cutout_info()["instances"] == 0
    opaque = make_ctx()
    load(opaque, moved, None)
    same_snapshot(snapshot(c, sc), snapshot(opaque, sc))
    opaque.close()
    c.set_material_cutouts(mtab)
    # skh_update_accel moving the card (the rays stay: they now cross it elsewhere -- off the grid, so hits are compared with a fresh context only)
    shift = S.translate((0.8, 0.0, -0.4))
    inst2 = np.array(marr["instances"], copy=True)
    card = cutref.card_instances(marr)[0]
    t = np.eye(4)
    t[:3, :] = np.asarray(inst2[card]["transform"], np.float64).reshape(3, 4)
    inst2[card]["transform"] = (shift @ t)[:3, :].astype(np.float32).reshape(12)
    c.update_accel(inst2)
    moved2, _, _ = cutref.card_scene(False, "single", cut_slot=2, xforms=[shift @ cutref.CARD_XFORMS["single"][0]])
    f = make_ctx()
    load(f, moved2, mtab)
    # (a ray that crosses the moved card on a cell edge could tell the two apart only through the hierarchy, which hit records do not depend on)
    same_snapshot(snapshot(c, sc), snapshot(f, sc))
    f.close()
    # skh_refit_accel after a vertex edit of the card: raised by 0.1
    arr3 = moved2.arrays()
    me = arr3["meshes"][int(arr3["instances"][card]["geom_id"])]
    v0, v1 = int(me["vertex_offset"]), int(me["vertex_offset"]) + int(me["vertex_count"])
    arr3["vertices"]["pos"][v0:v1, 1] += np.float32(0.1)
    c.set_geometry(arr3)
    c.refit_accel()
    f = make_ctx()
    f.set_scene(arr3)
    f.set_material_cutouts(mtab)
    same_snapshot(snapshot(c, sc), snapshot(f, sc))
    assert c.cutout_info()["instances"] == 1
    f.close(), c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8: curves beside cutouts
# ---------------------------------------------------------------------------------------------------------------------------------------------
def groom_scene(twin):
    """a 64-strand groom (the world-only curve kernel) with the card upright between it and the camera"""
    sc = scenes.hair_standin(seed=5, n_strands=64, n_cp=8)
    sc.mCurveWidths = [w * np.float32(50.0) for w in sc.mCurveWidths]  # (radii 0.02 ... 0.005: 64 strands thick enough for a few hundred of 4096 rays to meet one)
    alpha = cutref.block_alpha()
    tex = sc.addTexture(cutref.card_texture(alpha))
    mat = sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6), base_color_texture=tex)
    ids = cutref.add_card(sc, mat, alpha, twin, layout="front")
    return sc, (None if twin else cutref.table(mat + 1, {mat: cutref.entry(opacity_texture=tex, threshold=0.5)})), np.flatnonzero(cutref.card_kept(alpha)), ids


def test_curves_beside_cutouts():
    sc, tab, kept, ids = groom_scene(False)
    tw, _, _, _ = groom_scene(True)
    cm, ct = make_ctx(), make_ctx()
    arr = load(cm, sc, tab)
    load(ct, tw, None)
    curve = [k for k, i in enumerate(arr["instances"]) if int(i["type"]) == S.INSTANCE_CURVE]
    assert len(curve) == 1
    # through the card towards the head
    rays = cutref.card_rays("front", False, 4096)
    got, want = cm.trace(rays, 0), ct.trace(rays, 0)
    hits_equal(got, want, kept, ids)
    assert np.isin(got["instance_id"], ids).any() and (got["instance_id"] == 0).any()  # kept triangles; the scalp behind cut ones
    sh = np.array(rays, copy=True)
    sh["tmax"] = np.where(np.arange(len(sh)) % 2 == 0, 1.8, 3.5).astype(np.float32)  # ends behind the card | inside the head
    assert np.array_equal(cm.trace(sh, 1)["t"], ct.trace(sh, 1)["t"])
    # towards the strands: rays from every side at the shell the hair fills, those through the card's plane inside the card left out BY CONSTRUCTION
    # (origins at z <= 0.5, behind the card at z = 2.2, aimed at points of the shell: none reaches the card's plane)
    rs = np.random.RandomState(12)
    d = rs.normal(size=(4096, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = -np.abs(d[:, 2])
    org = d * 3.0 + np.array([0.0, 0.0, 0.4])
    tg = rs.normal(size=(4096, 3))
    tg = tg / np.linalg.norm(tg, axis=1, keepdims=True) * rs.uniform(1.0, 1.4, (4096, 1))
    hair = cutref.make_rays(org, tg)
    hair["tmax"] = (np.linalg.norm(tg - org, axis=1) + 0.3).astype(np.float32)  # (... and end 0.3 behind their target, at z < 1.8)
    assert (hair["origin"][:, 2] <= 0.5).all() and (tg[:, 2] <= 1.4).all()
    a = cm.trace(hair, 0)
    cm.set_material_cutouts(None)
    b = cm.trace(hair, 0)
    cm.set_material_cutouts(tab)
    assert a.tobytes() == b.tobytes() and (a["instance_id"] == curve[0]).sum() > 10
    assert a.tobytes() == ct.trace(hair, 0).tobytes()
    images_equal(render(cm, sc, 32, 32), render(ct, tw, 32, 32))
    assert cm.cutout_info()["continued_closest"] > 0
    cm.close(), ct.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 9: refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from strelka_amd import capi

    sc, tab, _ = cutref.card_scene(False, "single")
    c = make_ctx()
    load(c, sc, tab)
    want = render(c, sc, 32, 32)
    bad = []
    for field, value in (("opacity_channel", 4), ("opacity_scale", np.nan), ("opacity_bias", np.inf), ("threshold", 1.5), ("threshold", -0.1), ("threshold", np.nan)):
        t = np.array(tab, copy=True)
        t[field][1] = value
        bad.append(t)
    for k in range(3):
        t = np.array(tab, copy=True)
        t["reserved"][0, k] = 1
        bad.append(t)
    bad.append(cutref.table(3, {1: tab[1]}))  # more entries than materials
    for t in bad:
        st = c.lib.skh_set_material_cutouts(c.h, t.ctypes.data_as(capi.C.c_void_p), len(t))
        assert st == 3, (st, t)  # SKH_INVALID_ARGUMENT
        assert b"skh_set_material_cutouts" in c.lib.skh_last_error(c.h)
        images_equal(render(c, sc, 32, 32), want)  # the previous table is still in effect
    assert c.cutout_info()["instances"] == 1
    # a material that both emits and is cut: refused by the call that would use it, with its index; gone with either of the two
    le = np.zeros((2, 3), np.float32)
    le[1] = (1.0, 2.0, 3.0)
    c.set_emission(le)
    for call in (lambda: render(c, sc, 32, 32), lambda: c.trace(cutref.card_rays("single", False, 63), 0), lambda: c.cutout_info()):
        with pytest.raises(capi.SkhError, match="material 1 "):
            call()
    c.set_material_cutouts(None)
    assert np.isfinite(render(c, sc, 32, 32)[0]).all()
    c.set_material_cutouts(tab)
    with pytest.raises(capi.SkhError, match="material 1 "):
        render(c, sc, 32, 32)
    c.set_emission(None)
    images_equal(render(c, sc, 32, 32), want)
    # an emitter beside a cutout is fine
    le[0], le[1] = (0.5, 0.5, 0.5), 0.0
    c.set_emission(le)
    assert np.isfinite(render(c, sc, 32, 32)[0]).all()
    # cutout_rounds outside 1..32
    for v in (0, 33, -1):
        assert c.lib.skh_set_option(c.h, b"cutout_rounds", v) == 3
    for v in (1, 32, 8):
        assert c.lib.skh_set_option(c.h, b"cutout_rounds", v) == 0
    c.set_emission(None)
    images_equal(render(c, sc, 32, 32), want)
    c.close()
