"""Material textures on the GPU ("Material textures"): roughness, metallic / ORM and emission maps through
skh_set_material_textures.  The CPU checker knows none of it; the yardstick is tests/mtexref.py -- the look-up and resolve_material restated in numpy
float32 operation by operation (the library is built with -ffp-contract=off: bit equality is the bar), the emission at an emitter sample in float64 --
and, for the integrator, scenes in which the maps are PLATEAUS: with texel values 0 and 255 and all four texels of a footprint equal, the bilinear sum
is exactly 0 or 1 (the 1.8 fixed-point weights are multiples of 2^-16 that add up to 1), so a textured material must render the bits of a constant one."""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import emitref, mtexref
from tests import test_gpu_emit as E

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture
def ctx():
    from strelka_amd import build, capi

    build.build()
    c = capi.Context(0)
    yield c
    c.close()


def entry(**kw):
    e = np.zeros((), S.MATERIAL_TEXTURES)
    e["emission_channel"], e["roughness_scale"], e["metallic_scale"] = 4, 1.0, 1.0
    for k, v in kw.items():
        e[k] = v
    return e


def material(type_=S.MAT_PBR, base=(0.5, 0.5, 0.5), roughness=0.5, metallic=0.0, base_tex=0):
    m = np.zeros((), S.MATERIAL)
    m["type"], m["base_color"], m["roughness"], m["metallic"], m["specular"], m["ior"], m["base_color_texture"] = type_, base, roughness, metallic, 0.5, 1.5, base_tex
    return m


def add_uv_triangles(sc, tris, uvs, mat):
    """tris: (N, 3, 3) vertices, uvs: (N, 3, 2); triangle k of the mesh is tris[k]; flat normals"""
    t = np.asarray(tris, np.float32)
    vb, ib = S.deindex(t.reshape(-1, 3), np.arange(3 * len(t)).reshape(-1, 3))
    vb["uv"] = S.pack_uv(np.asarray(uvs, np.float32).reshape(-1, 2))
    return sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, ib), mat, np.eye(4))


def rect_tris(x0, x1, z0, z1, y, u0, u1, v0, v1, down=False):
    """an axis-parallel rectangle in the plane y as two triangles, u along x and v along z; `down`: winds towards -Y"""
    p = [(x0, y, z1), (x1, y, z1), (x1, y, z0), (x0, y, z0)]
    uv = [(u0, v1), (u1, v1), (u1, v0), (u0, v0)]
    idx = [0, 2, 1, 0, 3, 2] if down else [0, 1, 2, 0, 2, 3]
    return np.float32([p[i] for i in idx]).reshape(2, 3, 3), np.float32([uv[i] for i in idx]).reshape(2, 3, 2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1: the probe against mtexref, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def probe_cases():
    """textures: 1 = 5 x 3 (columns x rows), 2 = 4 x 4 -- non-square and not a power of two: the smallest that show a row / column swap or a wrong wrap.
    -> (materials, table, Le): every channel choice, scale / bias pairs that stay inside [0, 1] and that clamp at both ends, shared and distinct ids, slots
    alone, ids beyond the list, materials that are not PBR, base colour beside the maps, every emission mode, an emission map on a material that does not emit"""
    mats, tab, le = [], [], []

    def add(m, e, l=(0.0, 0.0, 0.0)):
        mats.append(m), tab.append(e), le.append(l)

    for c in range(4):  # distinct ids, every channel on both slots, inside [0, 1]
        add(material(), entry(roughness_texture=1, metallic_texture=2, roughness_channel=c, metallic_channel=3 - c, roughness_scale=0.5, roughness_bias=0.25,
                              metallic_scale=0.8, metallic_bias=0.1))
    add(material(), entry(roughness_texture=1, metallic_texture=1, roughness_channel=1, metallic_channel=2, roughness_scale=3.0, roughness_bias=-1.0,
                          metallic_scale=-2.5, metallic_bias=1.75))  # shared (ORM), clamps at both ends
    add(material(base_tex=1), entry(roughness_texture=2, metallic_texture=2, roughness_channel=3, metallic_channel=0, roughness_scale=0.3, roughness_bias=0.7,
                                    metallic_scale=1.0, metallic_bias=0.0))  # shared, the other texture, base colour from the first
    add(material(roughness=0.37), entry(metallic_texture=2, metallic_channel=1))  # metallic alone
    add(material(metallic=0.81), entry(roughness_texture=1, roughness_channel=2, roughness_scale=0.7, roughness_bias=0.1))  # roughness alone
    add(material(roughness=0.21), entry(roughness_texture=3, metallic_texture=2, metallic_channel=2))  # an id beyond the list = none
    for t in (S.MAT_DIFFUSE, S.MAT_GLASS):  # not PBR: roughness / metallic stay, emission applies
        add(material(t, roughness=0.3, metallic=0.6), entry(roughness_texture=1, metallic_texture=2, emission_texture=2, emission_channel=4), (3.0, 2.0, 1.0))
    for c in range(5):  # every emission mode, on both textures
        add(material(base_tex=2), entry(emission_texture=1 + c % 2, emission_channel=c), (0.5 + c, 4.0, 7.5 - c))
    add(material(), entry(roughness_texture=2, emission_texture=1, emission_channel=4), (0.0, 0.0, 0.0))  # Le = 0 does not emit, whatever its map
    add(material(base_tex=2), entry())  # nothing bound: base colour alone
    return np.array(mats, S.MATERIAL), np.array(tab, S.MATERIAL_TEXTURES), np.float32(le)


def probe_uvs():
    rs = np.random.RandomState(7)
    lattice = np.stack(np.meshgrid(np.arange(-10, 21) / 10.0, np.arange(-6, 13) / 6.0, indexing="ij"), -1).reshape(-1, 2)  # texel centres and edges of 5 x 3, wrapped
    uv = np.concatenate([rs.uniform(-2, 3, (192, 2)), lattice[rs.permutation(len(lattice))[:56]], [[0, 0], [1, 1], [0.125, 0.875], [-0.125, 0.375], [0.999999, 1e-7], [-1e-8, 2.5],
                                                                                                  [0.5, 0.5], [0.3, 0.5]]]).astype(np.float32)
    assert len(uv) == 256
    return uv


def test_probe_equals_the_restatement_bit_for_bit(ctx):
    rs = np.random.RandomState(3)
    textures = [rs.randint(0, 256, (3, 5, 4)).astype(np.uint8), rs.randint(0, 256, (4, 4, 4)).astype(np.uint8)]
    mats, tab, le = probe_cases()
    uv = probe_uvs()
    ctx.set_textures(textures)
    ctx.set_materials(mats)
    ctx.set_emission(le)
    ctx.set_material_textures(tab)
    mid = np.repeat(np.arange(len(mats)), len(uv)).astype(np.uint32)
    got = ctx.material_probe(mid, np.tile(uv, (len(mats), 1))).reshape(len(mats), len(uv), 8)
    for k in range(len(mats)):
        want = mtexref.resolve_material(mats[k], tab[k], le[k], textures, uv)
        bad = np.argwhere(got[k].view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (k, tab[k], bad[:4], got[k][bad[:4, 0]], want[bad[:4, 0]])
    # the cases do what they are there for: values strictly inside (0, 1) and clamped at both ends, maps that change something
    assert (got[4, :, 3] == 0).any() and (got[4, :, 3] == 1).any() and (got[4, :, 4] == 0).any() and (got[4, :, 4] == 1).any()
    assert ((got[0, :, 3] > 0.25) & (got[0, :, 3] < 0.75)).any()
    assert (got[8, :, 3] == F(0.21)).all() and (got[9, :, 3] == F(0.3)).all() and (got[9, :, 4] == F(0.6)).all()
    assert (got[16, :, 5:] == 0).all() and (got[9, :, 5:] != np.float32([3, 2, 1])).any()
    # without the table: base colour alone, the constants, the material's Le
    ctx.set_material_textures(None)
    plain = ctx.material_probe(mid, np.tile(uv, (len(mats), 1))).reshape(len(mats), len(uv), 8)
    for k in range(len(mats)):
        assert np.array_equal(plain[k].view(np.uint32), mtexref.resolve_material(mats[k], None, le[k], textures, uv).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2: plateau equivalence
# ---------------------------------------------------------------------------------------------------------------------------------------------
def plateau_texture():
    """8 x 8, every channel its own 0 / 255 pattern of 4 x 4 blocks: r by column, g by row, b = r xor g, a = not r"""
    t = np.zeros((8, 8, 4), np.uint8)
    yy, xx = np.mgrid[0:8, 0:8]
    t[..., 0] = np.where(xx < 4, 255, 0)
    t[..., 1] = np.where(yy < 4, 255, 0)
    t[..., 2] = np.where((xx < 4) != (yy < 4), 255, 0)
    t[..., 3] = np.where(xx < 4, 0, 255)
    return t


# uvs inside one plateau, at least one texel from its edge (texel centres 1 ... 2 of a block 0 ... 3 and 5 ... 6 of 4 ... 7: u in [1.5, 2.5] / 8 and [5.5, 6.5] / 8)
UV_A, UV_B = (0.2, 0.3, 0.2, 0.3), (0.7, 0.8, 0.2, 0.3)  # (u0, u1, v0, v1): A sees r g b a = 1 1 0 0, B sees 0 1 1 1


def two_quads(mat_a, mat_b, textures=(), uv_a=UV_A, uv_b=UV_B, table=None, materials=None, distant=False):
    """two quads side by side on the floor plane in front of a grey wall (something for their reflections to show), one rect light above (`distant`: a
    distant light instead -- no proxy geometry for rays to hit)"""
    sc = S.Scene()
    for t in textures:
        sc.addTexture(t)
    for kw in materials:
        sc.addMaterial(**kw)
    wall = sc.addMaterial(S.MAT_DIFFUSE, (0.7, 0.6, 0.5))
    add_uv_triangles(sc, *rect_tris(-1.1, -0.1, -0.5, 0.5, 0.0, *uv_a), mat_a)
    add_uv_triangles(sc, *rect_tris(0.1, 1.1, -0.5, 0.5, 0.0, *uv_b), mat_b)
    E.add_triangles(sc, np.float32([[(-2, 0, -0.6), (2, 0, -0.6), (2, 2, -0.6)], [(-2, 0, -0.6), (2, 2, -0.6), (-2, 2, -0.6)]]), wall)
    if distant:
        sc.createLight({"type": 3, "useXform": False, "position": (0.0, 0.0, 0.0), "orientation": (-60.0, 20.0, 0.0), "halfAngle": math.radians(5.0), "intensity": 3.0,
                        "color": (1.0, 1.0, 1.0), "radius": 0.0})
    else:
        sc.createLight({"type": 0, "useXform": False, "position": (0.0, 2.0, 0.3), "orientation": (-90.0, 0.0, 0.0), "width": 1.5, "height": 1.0,
                        "color": (1.0, 1.0, 1.0), "intensity": 30.0})
    cam = S.Camera(fov=45.0)
    cam.lookAt((0.0, 1.6, 2.6), (0.0, 0.2, 0.0))
    sc.addCamera(cam)
    arr = sc.arrays()
    if table is not None:
        arr["material_textures"] = table
    return sc, arr


def affine(s, t, b):
    """clamp01(fl(fl(s t) + b))"""
    return float(mtexref.clamp01(F(F(F(s) * F(t)) + F(b))))


@pytest.mark.parametrize("rs,rb,ms,mb", [(0.5, 0.25, 0.8, 0.1), (2.0, 0.1, -1.0, 0.5)])  # inside [0, 1]; clamping above (roughness) and below (metallic)
def test_plateau_maps_render_the_bits_of_constant_materials(ctx, rs, rb, ms, mb):
    """ONE material with a roughness map (channel r) and a metallic map (channel b, the same texture: one look-up) against TWO constant materials.
    Quad A sees r = 1, b = 0, quad B r = 0, b = 1.  A channel mix-up, a dropped clamp or an fma changes the bits."""
    base = dict(type=S.MAT_PBR, base_color=(0.8, 0.5, 0.3), specular=0.5)
    ra, rb_, ma, mb_ = affine(rs, 1.0, rb), affine(rs, 0.0, rb), affine(ms, 0.0, mb), affine(ms, 1.0, mb)
    assert len({ra, rb_}) == 2 and len({ma, mb_}) == 2
    for bake in (4, 0):
        ctx.set_option("bake_world", bake)
        sc, arr = two_quads(0, 0, [plateau_texture()], materials=[dict(base, roughness=0.9, metallic=0.9, roughness_texture=1, metallic_texture=1, roughness_channel=0,
                                                                       metallic_channel=2, roughness_scale=rs, roughness_bias=rb, metallic_scale=ms, metallic_bias=mb)])
        assert "material_textures" in arr
        ctx.set_scene(arr)
        got = E.render(ctx, sc, 32, 24, 4)
        sc2, arr2 = two_quads(0, 1, materials=[dict(base, roughness=ra, metallic=ma), dict(base, roughness=rb_, metallic=mb_)])
        assert "material_textures" not in arr2
        ctx.set_scene(arr2)
        want = E.render(ctx, sc2, 32, 24, 4)
        assert np.isfinite(want).all() and want.max() > 0
        assert np.array_equal(got, want), (bake, np.abs(got - want).max())
        # ... and the maps are seen: swapping the two constant materials gives another image
        sc3, arr3 = two_quads(1, 0, materials=[dict(base, roughness=ra, metallic=ma), dict(base, roughness=rb_, metallic=mb_)])
        ctx.set_scene(arr3)
        assert not np.array_equal(E.render(ctx, sc3, 32, 24, 4), want)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3: scheduling and hierarchy options
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_options_leave_a_mapped_image_bit_identical(ctx):
    """speculation, sub-frame batches, env_nee / emit_nee with neither an environment nor an emitter -- and bake_world 4 / 0: the option is part of the intersection's
    definition (a baked instance is intersected in world space), so the scene is one in which both definitions give the same bits: every mesh instance under
    the identity transform, and a distant light, which has no proxy geometry"""
    tex = np.random.RandomState(9).randint(0, 256, (4, 4, 4)).astype(np.uint8)
    base = dict(type=S.MAT_PBR, base_color=(0.8, 0.5, 0.3), metallic=0.5)
    uv = (0.0, 2.0, 0.0, 1.0)
    mapped = [dict(base, roughness=0.5, roughness_texture=1, roughness_channel=1, roughness_scale=0.8, roughness_bias=0.1)]
    w, h, spp = 32, 24, 4
    images = []
    for bake in (4, 0):
        ctx.set_option("bake_world", bake)
        sc, arr = two_quads(0, 0, [tex], uv, uv, materials=mapped, distant=True)
        ctx.set_scene(arr)
        ctx.set_option("speculate", 0)
        images.append(E.render(ctx, sc, w, h, spp))
        ctx.set_option("speculate", 8)
        images.append(E.render(ctx, sc, w, h, spp))
        for b in (1, 3):
            ctx.set_option("subframe_batch", b)
            ctx.resize(w, h)
            ctx.render_subframes(S.frame_params(sc.getCamera(), w, h, subframe_index=0, spp_total=spp, max_depth=4), spp)
            images.append(ctx.read_accum()[..., :3].copy())
        ctx.set_option("subframe_batch", 0)
        for opt in ("env_nee", "emit_nee"):  # neither an environment nor an emitter is there
            ctx.set_option(opt, 0)
            images.append(E.render(ctx, sc, w, h, spp))
            ctx.set_option(opt, 1)
    assert images[0].max() > 0 and np.isfinite(images[0]).all()
    for k, im in enumerate(images[1:]):
        assert np.array_equal(im, images[0]), k + 1
    # the gradient is seen: neither constant extreme gives this image
    for t in (0.0, 1.0):
        sc, arr = two_quads(0, 0, [tex], uv, uv, materials=[dict(base, roughness=affine(0.8, t, 0.1))], distant=True)
        ctx.set_scene(arr)
        assert not np.array_equal(E.render(ctx, sc, w, h, spp), images[0])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4: nothing changes without it
# ---------------------------------------------------------------------------------------------------------------------------------------------
def textured_floor():
    """a floor quad with uvs 0 ... 2 and a base-colour checker under a rect light (the scene of tests/test_textures.py, built here: that module needs the CPU checker)"""
    t = np.zeros((8, 8, 4), np.uint8)
    yy, xx = np.mgrid[0:8, 0:8]
    t[(xx + yy) % 2 == 0] = (230, 40, 40, 255)
    t[(xx + yy) % 2 == 1] = (40, 40, 230, 255)
    sc = S.Scene()
    sc.addMaterial(S.MAT_PBR, (0.7, 0.7, 0.7), roughness=0.6, metallic=0.0, base_color_texture=sc.addTexture(t))
    add_uv_triangles(sc, *rect_tris(-2.0, 2.0, -2.0, 2.0, 0.0, 0.0, 2.0, 0.0, 2.0), 0)
    sc.createLight({"type": 0, "useXform": False, "position": (0.0, 3.0, 0.0), "orientation": (-90.0, 0.0, 0.0), "width": 1.5, "height": 1.5,
                    "color": (1.0, 1.0, 1.0), "intensity": 30.0})
    cam = S.Camera(fov=45.0)
    cam.lookAt((0.0, 3.0, 4.5), (0.0, 0.0, 0.0))
    sc.addCamera(cam)
    return sc


@pytest.mark.parametrize("which", ["cornell", "textured"])
def test_nothing_changes_without_a_table(ctx, which):
    from strelka_amd import capi

    sc = scenes.cornell_box() if which == "cornell" else textured_floor()
    arr = sc.arrays()
    never = capi.Context(0)
    try:
        never.set_scene(arr)
        want = E.render(never, sc, 32, 24, 4)
    finally:
        never.close()
    assert want.max() > 0
    ctx.set_scene(arr)
    nm = len(arr["materials"])
    zeros = np.array([entry()] * nm, S.MATERIAL_TEXTURES)
    ctx.set_material_textures(zeros)  # a table whose ids are all 0 equals no table
    assert np.array_equal(E.render(ctx, sc, 32, 24, 4), want)
    if which == "textured":
        live = zeros.copy()
        live["roughness_texture"], live["roughness_scale"], live["roughness_bias"] = 1, 0.5, 0.1
        ctx.set_material_textures(live)
        assert not np.array_equal(E.render(ctx, sc, 32, 24, 4), want)
    else:
        beyond = zeros.copy()
        beyond["roughness_texture"] = beyond["metallic_texture"] = beyond["emission_texture"] = 5  # the scene has no texture at all
        ctx.set_material_textures(beyond)
        assert np.array_equal(E.render(ctx, sc, 32, 24, 4), want)
    ctx.set_material_textures(None)  # had a table, removed it
    assert np.array_equal(E.render(ctx, sc, 32, 24, 4), want)
    ctx.set_material_textures(None)  # (removing nothing is fine)
    assert np.array_equal(E.render(ctx, sc, 32, 24, 4), want)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5: emission at depth 0
# ---------------------------------------------------------------------------------------------------------------------------------------------
LE = np.float32([10.0, 6.0, 3.0])


def halves_texture():
    """8 x 8: columns 0 ... 3 white, 4 ... 7 black (every channel)"""
    t = np.zeros((8, 8, 4), np.uint8)
    t[:, :4] = 255
    return t


def plane_points(sc, w, h, y):
    """where the rays through the pixels' corners meet the plane of height y: (h, w, 4, 3), generate_camera_ray in float64"""
    p = S.frame_params(sc.getCamera(), w, h)
    V, Cm = np.asarray(p["view_to_world"], np.float64).reshape(4, 4), np.asarray(p["clip_to_view"], np.float64).reshape(4, 4)
    out = np.zeros((h, w, 4, 3))
    o = (V @ [0, 0, 0, 1])[:3]
    for py in range(h):
        for px in range(w):
            for k, (jx, jy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                vs = Cm @ np.array([(px + jx) / w * 2 - 1, (py + jy) / h * 2 - 1, 1.0, 1.0])
                d = (V @ [vs[0], vs[1], vs[2], 0.0])[:3]
                out[py, px, k] = o + d * ((y - o[1]) / d[1])
    return out


def test_emission_map_seen_by_the_camera(ctx):
    """The camera looks straight up at a black emissive 1.0 x 0.6 quad whose uvs run over u = 1/8 ... 7/8: the map is exactly 1 for u in [1/16, 7/16] and exactly 0
    for u in [9/16, 15/16] (footprints inside one half).  1 spp, depth 0 hits: a pixel wholly inside the lit part holds Le through the accumulate step's
    known arithmetic, one wholly inside the dark part 0."""
    sc = S.Scene()
    sc.addTexture(halves_texture())
    lamp = sc.addMaterial(S.MAT_DIFFUSE, (0.0, 0.0, 0.0), emission=tuple(float(v) for v in LE), emission_texture=1)
    add_uv_triangles(sc, *rect_tris(-0.5, 0.5, -0.3, 0.3, 1.5, 0.125, 0.875, 0.125, 0.875, down=True), lamp)
    cam = S.Camera(fov=40.0)
    cam.lookAt((0.0, 0.2, 0.0), (0.0, 1.5, 0.01))
    sc.addCamera(cam)
    ctx.set_scene(sc.arrays())
    w, h = 32, 24
    ctx.resize(w, h)
    ctx.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=0, spp_total=1, max_depth=2))
    img = ctx.read_accum()[..., :3]
    pts = plane_points(sc, w, h, 1.5)
    u = 0.125 + 0.75 * (pts[..., 0] + 0.5)
    on_quad = (np.abs(pts[..., 0]) < 0.49).all(-1) & (np.abs(pts[..., 2]) < 0.29).all(-1)
    m = 2e-3  # (the 16-bit uv of a vertex is off by up to 6e-4)
    lit = on_quad & (u > 1 / 16 + m).all(-1) & (u < 7 / 16 - m).all(-1)
    dark = on_quad & (u > 9 / 16 + m).all(-1) & (u < 15 / 16 - m).all(-1)
    assert lit.sum() >= 40 and dark.sum() >= 40, (lit.sum(), dark.sum())
    e = np.ascontiguousarray(S.default_exposure(), np.float32)
    want = E.f32(ctx.unit_probe("accumulate", LE.reshape(1, 3).copy(), param=0, consts=e))[0]
    assert (want > 0).all()
    assert np.array_equal(img[lit].view(np.uint32), np.broadcast_to(want, img[lit].shape).copy().view(np.uint32))
    assert (img[dark] == 0).all()
    # without the map the whole quad shows Le
    ctx.set_material_textures(None)
    ctx.render_subframe(S.frame_params(sc.getCamera(), w, h, subframe_index=0, spp_total=1, max_depth=2))
    img = ctx.read_accum()[..., :3]
    assert np.array_equal(img[lit | dark].view(np.uint32), np.broadcast_to(want, img[lit | dark].shape).copy().view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6: the emitter sample
# ---------------------------------------------------------------------------------------------------------------------------------------------
def emitter_mesh(plateau):
    """the 1.0 x 0.6 quad at height 1.5, facing down, as 8 x 4 cells; uvs: `plateau`: cells of the left half inside the lit part of halves_texture, the
    others inside the dark part; else one map over the quad, 1.5 times in u (it wraps) and once in v"""
    nx, nz = 8, 4
    tris, uvs = [], []
    for i in range(nx):
        for j in range(nz):
            x0, x1, z0, z1 = i / nx - 0.5, (i + 1) / nx - 0.5, (j / nz - 0.5) * 0.6, ((j + 1) / nz - 0.5) * 0.6
            if plateau:
                c = 0.2 if i < nx // 2 else 0.7
                uv = (c + 0.01 * i, c + 0.01 * (i + 1), 0.3 + 0.02 * j, 0.3 + 0.02 * (j + 1))
            else:
                uv = (1.5 * i / nx, 1.5 * (i + 1) / nx, j / nz, (j + 1) / nz)
            t, q = rect_tris(x0, x1, z0, z1, 1.5, *uv, down=True)
            tris.append(t), uvs.append(q)
    return np.concatenate(tris), np.concatenate(uvs)


def sample_probe(ctx, u, ux, uy, P):
    rec = np.zeros((len(u), 6), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3:6] = u, ux, uy, P
    return ctx.emitter_probe("sample", rec)


@pytest.mark.parametrize("plateau", [True, False])
def test_emitter_sample_carries_the_map(ctx, plateau):
    """SKH_EMIT_PROBE_SAMPLE.  Plateau maps: Le is exactly the material's or 0, by the half the sampled triangle lies in.  A random 4 x 4 rgb map: against the float64
    restatement, |dLe| <= Le D / 256 per channel, D the largest difference between neighbouring texels -- the uv interpolated in float32 can move one
    fixed-point weight by one step of 1 / 256 and no more.  Point, normal, pdf, dist and ids are the bits of the same call without the map."""
    tex = halves_texture() if plateau else np.random.RandomState(21).randint(0, 256, (4, 4, 4)).astype(np.uint8)
    tris, uvs = emitter_mesh(plateau)
    sc = S.Scene()
    sc.addTexture(tex)
    grey = sc.addMaterial(S.MAT_DIFFUSE, (0.5, 0.5, 0.5))
    lamp = sc.addMaterial(S.MAT_DIFFUSE, (0.0, 0.0, 0.0), emission=tuple(float(v) for v in LE), emission_texture=1, emission_channel=4)
    E.add_triangles(sc, np.float32([[(-2, 0, 2), (2, 0, 2), (2, 0, -2)]]), grey)
    inst = add_uv_triangles(sc, tris, uvs, lamp)
    sc.addCamera(S.Camera())
    arr = sc.arrays()
    ctx.set_scene(arr)
    assert ctx.emitter_info()["triangles"] == len(tris) == 64
    rs = np.random.RandomState(4)
    n = 4096
    u, ux, uy = (rs.rand(n).astype(np.float32) for _ in range(3))
    P = (rs.rand(n, 3) * [2, 1, 2] - [1, 0, 1]).astype(np.float32)
    o = sample_probe(ctx, u, ux, uy, P)
    ctx.set_material_textures(None)
    o0 = sample_probe(ctx, u, ux, uy, P)
    assert np.array_equal(o[:, :6], o0[:, :6]) and np.array_equal(o[:, 9:], o0[:, 9:])
    assert np.array_equal(E.f32(o0[:, 6:9]), np.broadcast_to(LE, (n, 3)))
    assert (o[:, 11] == inst).all()
    prim = o[:, 12].astype(np.int64)
    assert len(np.unique(prim)) == 64
    got = E.f32(o[:, 6:9])
    if plateau:
        lit = (prim // 2) // 4 < 4  # cell (i, j) = triangles 2 (4 i + j), + 1
        assert lit.any() and (~lit).any()
        assert np.array_equal(got[lit], np.broadcast_to(LE, got[lit].shape)) and (got[~lit] == 0).all()
        return
    # the vertices' uvs as the device unpacks them, then float64
    mesh = arr["meshes"][arr["instances"][inst]["geom_id"]]
    packed = arr["vertices"]["uv"][int(mesh["vertex_offset"]):int(mesh["vertex_offset"]) + int(mesh["vertex_count"])]
    uu, vv = mtexref.unpack_uv(packed)
    tri_uv = np.stack([uu, vv], -1).astype(np.float64).reshape(-1, 3, 2)[prim]
    want = mtexref.emission_at_sample(LE, tex, 4, tri_uv, ux, uy)
    D = mtexref.neighbour_difference(tex, [0, 1, 2])
    err = np.abs(got.astype(np.float64) - want) / LE.astype(np.float64)
    print(f"emission at the sample: max |dLe| / Le = {err.max():.3e} (bar D / 256 = {D / 256:.3e}); {int((err > 1e-6).sum())} of {n} samples moved a weight")
    assert D > 0.5 and (err <= D / 256).all()
    assert np.abs(want / LE - 0.5).mean() > 0.1  # (the map is seen)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7: the closed form
# ---------------------------------------------------------------------------------------------------------------------------------------------
LIT_HALF = np.array([(-0.5, 1.5, -0.3), (0.0, 1.5, -0.3), (0.0, 1.5, 0.3), (-0.5, 1.5, 0.3)])  # the x < 0 half of tests/test_gpu_emit.py's QUAD, wound towards -Y


@pytest.mark.parametrize("view", ["under", "off_axis"])
def test_floor_under_a_half_lit_quad_has_its_closed_form(ctx, view):
    """tests/test_gpu_emit.py's floor under its black 1.0 x 0.6 emissive quad, the quad cut by plateau maps into a lit half (x < 0) and a dark one: a pixel's
    expectation is rho Le E(p) / pi with E Lambert's polygon formula over the LIT half only.  One launch of N samples, the mean over the 64 pixels, per
    channel: |mean - mu| <= 6 sqrt(V / (P N)) + eps(N) mu + spread, V <= mu (2 rho Le - mu) -- a sample weighted by the map still lies in [0, 2 rho Le] --,
    N the smallest power of two that puts the bound below 10 % of mu.  The table's weights are the material's: with emit_nee 1 half of the picks land on the
    dark half and return nothing, and the estimator must still be right."""
    sc = S.Scene()
    sc.addTexture(halves_texture())
    grey = sc.addMaterial(S.MAT_DIFFUSE, (E.RHO, E.RHO, E.RHO))
    lamp = sc.addMaterial(S.MAT_DIFFUSE, (0.0, 0.0, 0.0), emission=tuple(float(v) for v in E.LE), emission_texture=1, emission_channel=4)
    E.add_triangles(sc, np.float32([[(-20, 0, 20), (20, 0, 20), (20, 0, -20)], [(-20, 0, 20), (20, 0, -20), (-20, 0, -20)]]), grey)
    tl, ul = rect_tris(-0.5, 0.0, -0.3, 0.3, 1.5, 0.2, 0.3, 0.2, 0.3, down=True)
    td, ud = rect_tris(0.0, 0.5, -0.3, 0.3, 1.5, 0.7, 0.8, 0.2, 0.3, down=True)
    add_uv_triangles(sc, np.concatenate([tl, td]), np.concatenate([ul, ud]), lamp)
    cam = S.Camera(fov=1.5)
    cam.lookAt(*E.VIEWS[view])
    sc.addCamera(cam)
    ctx.set_scene(sc.arrays())
    assert ctx.emitter_info()["triangles"] == 4
    fpts = E.floor_points(sc, 8, 8)
    Ep = np.array([[[emitref.polygon_irradiance(LIT_HALF, fpts[y, x, k], (0, 1, 0)) for k in range(5)] for x in range(8)] for y in range(8)])
    whole = np.array([[emitref.polygon_irradiance(E.QUAD, fpts[y, x, 0], (0, 1, 0)) for x in range(8)] for y in range(8)])
    assert 0.2 < Ep[:, :, 0].mean() / whole.mean() < 0.8  # (the dark half would be seen: the whole quad gives another number)
    rl = E.RHO * E.LE.astype(np.float64)
    mu = (Ep[:, :, 0, None] * rl / np.pi).mean(axis=(0, 1))
    spread = np.abs(Ep[:, :, 1:] - Ep[:, :, :1]).max(axis=2).mean() * rl / np.pi
    Pn = 64
    V = mu * (2 * rl - mu)
    bound_of = lambda n: 6 * np.sqrt(V / (Pn * n)) + E.eps(n) * mu + spread
    N = 256
    while not (bound_of(N) <= 0.1 * mu).all() and N < 2 ** 20:
        N *= 2
    bound = bound_of(N)
    assert (bound <= 0.1 * mu).all() and N <= 2 ** 17, (N, bound / mu)
    for nee in (0, 1):
        ctx.set_option("emit_nee", nee)
        ctx.reset_stats()
        img = E.one_launch(ctx, sc, N, 2)
        mean = img.mean(axis=(0, 1))
        print(f"{view} emit_nee {nee}: N {N}, mean {mean}, mu {mu}, |diff| / bound {np.abs(mean - mu) / bound}, bound / mu {bound / mu}, shadow rays {ctx.stats()['rays_shadow']}")
        assert (np.abs(mean - mu) <= bound).all(), (nee, mean, mu, bound)
        assert (ctx.stats()["rays_shadow"] > 0) == bool(nee)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8: bad input
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_and_the_previous_table_stays(ctx):
    from strelka_amd import capi

    tex = np.random.RandomState(9).randint(0, 256, (4, 4, 4)).astype(np.uint8)
    uv = (0.0, 2.0, 0.0, 1.0)
    sc, arr = two_quads(0, 0, [tex], uv, uv, materials=[dict(type=S.MAT_PBR, base_color=(0.8, 0.5, 0.3), metallic=0.5, roughness=0.5)])
    nm = len(arr["materials"])
    good = np.array([entry()] * nm, S.MATERIAL_TEXTURES)
    good[0] = entry(roughness_texture=1, roughness_channel=1, roughness_scale=0.8, roughness_bias=0.1)
    ctx.set_scene(arr)
    plain = E.render(ctx, sc, 32, 24, 2)
    ctx.set_material_textures(good)
    a = E.render(ctx, sc, 32, 24, 2)
    assert not np.array_equal(a, plain) and np.isfinite(a).all()

    def edited(**kw):
        t = good.copy()
        for k, v in kw.items():
            t[k][0] = v
        return t

    cases = [edited(roughness_channel=4), edited(metallic_channel=7), edited(emission_channel=5), edited(roughness_scale=np.nan), edited(metallic_bias=np.inf),
             edited(reserved=(0, 1)), np.concatenate([good, good[:1]])]
    for bad in cases:
        with pytest.raises(capi.SkhError) as ei:
            ctx.set_material_textures(bad)
        assert "(3)" in str(ei.value)  # SKH_INVALID_ARGUMENT
        assert np.array_equal(E.render(ctx, sc, 32, 24, 2), a)  # the previous table still renders the previous bits
    # an id beyond the texture list behaves as 0
    ctx.set_material_textures(edited(roughness_texture=2))
    assert np.array_equal(E.render(ctx, sc, 32, 24, 2), plain)
    ctx.set_material_textures(edited(roughness_texture=2, metallic_texture=1, metallic_channel=3, metallic_scale=0.5))
    b = E.render(ctx, sc, 32, 24, 2)
    ctx.set_material_textures(edited(roughness_texture=0, metallic_texture=1, metallic_channel=3, metallic_scale=0.5))
    assert np.array_equal(E.render(ctx, sc, 32, 24, 2), b) and not np.array_equal(b, plain)
