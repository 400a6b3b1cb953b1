"""The first-hit AOV pass on the device (skh_render_aovs; DESIGN.md section 2, "First-hit AOVs").

The yardsticks: the renderer's own `debug = 1` view and raw queries (bit for bit), the CPU checker's trace() (bit for bit), tests/hitref.py and tests/aovref.py
(float64, under their written-out bounds), skh_material_probe and tests/mtexref.py (albedo, texture coordinates).  Every test calls the new entry point, so each
fails without the feature.  96 x 72 -- tests/test_hit_cpu.py's W, H -- unless a test says otherwise.

Figures of the float64 tests on an MI355X (worst error / bound over all scenes; docs/LOG.md has the table): see test_float64_*'s printed lines."""
import functools

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes
from tests import aovref, cutref, hitref, mtexref
from tests import test_hit_cpu as T

pytestmark = pytest.mark.gpu

W, H = T.W, T.H
F = np.float32
ALL = S.AOV_PLANES
CENTRE_EXCLUDED = ("smooth-mirror", "tilted-identity", "map-mirror-255-128-128", "map-mirror-128-255-128", "map-mirror-200-60-230")  # the quad's diagonal runs through pixel centres


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


def load(make, arr, w=W, h=H, **options):
    c = make(**options)
    c.set_scene(arr)
    c.resize(w, h)
    return c


def centre_jitter():
    return np.full((H, W, 2), 0.5, F)


@functools.lru_cache(maxsize=None)
def scene_of(name):
    """(scene, arrays, debug params, aov params, normal-map texel, has curves) of a scene of tests/test_hit_cpu.py, built once"""
    build, texel, curves = T.SCENES[name]
    sc = build()
    return sc, sc.arrays(), T.debug_params(sc), S.aov_params(sc.getCamera(), W, H), texel, curves


@functools.lru_cache(maxsize=None)
def rays_of(name, mode):
    """the float32 camera rays of a scene, flat: mode "centre" or "sample0" """
    _, _, params, _, _, _ = scene_of(name)
    o, d = hitref.camera_rays(params, W, H, 0, centre_jitter() if mode == "centre" else T.jitter())
    return o.reshape(-1, 3), d.reshape(-1, 3)


def reference_view(arr, rays, need_share):
    """T.reference_view for given rays: the classes of pixels from float64 alone.  `need_share`: the share of the frame that must hit"""
    hit = hitref.first_hits(arr, rays)
    clr, cinst, cwhere = hitref.curve_clearance(arr, rays)
    found = hit["inst"] >= 0
    curve_unclear = np.abs(clr) <= hitref.CURVE_EDGE
    curve = clr < -hitref.CURVE_EDGE
    assert (~curve | ~found | (cwhere < hit["t"])).all()
    hits_any = found | (clr < 0)
    excluded = hit["unclear"] | curve_unclear
    v = {"rays": rays, "hit": hit, "curve": curve & ~excluded, "curve_instance": cinst, "tri": found & ~curve & ~excluded, "miss": ~found & ~(clr < 0) & ~excluded,
         "excluded": excluded, "hits_any": hits_any}
    share, lost = hits_any.mean(), excluded.sum() / max(1, hits_any.sum())
    print(f"reference: {share:.1%} of the frame hits something, {lost:.2%} of that excluded")
    assert share >= need_share and lost <= 0.01
    return v


@functools.lru_cache(maxsize=None)
def view_of(name, mode):
    _, arr, params, _, _, _ = scene_of(name)
    if mode == "sample0":
        return T.reference_view(arr, params)  # (its own conditions: >= 0.40 of the frame hits, <= 0.01 of the hits excluded)
    o, d = rays_of(name, mode)
    return reference_view(arr, (o.reshape(H, W, 3), d.reshape(H, W, 3)), 0.40)


def aovs(c, ap, mode, planes=ALL, region=None):
    return c.render_aovs(ap, planes, region=region, sample_index=None if mode == "centre" else 0, spp_total=64)


def device_image(c, params, w=W, h=H):
    import torch

    img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    c.render_subframe(params, img.data_ptr())
    c.synchronize()
    return img.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1: jittered mode equals the renderer
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.SCENES))
def test_sample_mode_equals_the_normals_view(ctx, name):
    """(NORMAL + 1) / 2 in float32 equals the `debug = 1` image of sample 0 on every surface pixel, bit for bit, under the options that change how a hit reaches
    its shading records.  (A light proxy shows the light's radiance in that view, not a normal: kind 3 is left out; a miss is black there and 0 here.)"""
    sc, arr, params, ap, texel, curves = scene_of(name)
    for opt in [{}, {"bake_world": 0}, {"direct_records": 0}, {"compact_hits": 0}] + ([{"world_kernel": 0}] if curves else []):
        c = load(ctx, arr, **opt)
        p = aovs(c, ap, "sample0", ("ids", "normal"))
        kind = p["ids"][..., 3]
        surf = (kind == 1) | (kind == 2)
        img = device_image(c, params)[..., :3]
        assert surf.mean() >= 0.4 and ((kind == 2).any() == curves)
        assert np.array_equal(bits(aovref.normals_view(p["normal"], kind)[surf]), bits(img[surf])), opt
        assert (img[kind == 0] == 0).all() and (p["normal"][kind == 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2: the planes equal the raw query of the same rays
# ---------------------------------------------------------------------------------------------------------------------------------------------
def check_against_records(p, rec, arr):
    """IDS and HIT (t, u, v) against hit records of the same rays (the device's raw query, or the checker's): exact"""
    ids, thit = aovref.ids_and_hit(arr, rec)
    assert np.array_equal(p["ids"].reshape(-1, 4), ids)
    assert np.array_equal(bits(p["hit"].reshape(-1, 4)[:, :3]), bits(thit))


@pytest.mark.parametrize("mode", ["centre", "sample0"])
@pytest.mark.parametrize("name", list(T.SCENES))
def test_planes_equal_the_raw_query(ctx, name, mode):
    sc, arr, params, ap, texel, curves = scene_of(name)
    o, d = rays_of(name, mode)
    c = load(ctx, arr)
    p = aovs(c, ap, mode, ("ids", "hit"))
    check_against_records(p, c.trace(T.ray_records(o, d), 0), arr)
    check_against_records(p, T.oracle_for(arr).trace(T.ray_records(o, d), 0), arr)
    kinds = set(np.unique(p["ids"][..., 3]))
    assert kinds <= {0, 1, 2} and 1 in kinds and ((2 in kinds) == curves)


def scene_rays(sc, mode):
    params = S.frame_params(sc.getCamera(), W, H)
    o, d = hitref.camera_rays(params, W, H, 0, centre_jitter() if mode == "centre" else T.jitter())
    return o.reshape(-1, 3), d.reshape(-1, 3)


@pytest.mark.parametrize("mode", ["centre", "sample0"])
def test_cutout_holes_pick_what_is_behind(ctx, mode):
    """cutref.card_scene() with its cutout table: the planes are the raw query's, which honours the table -- a hole names the floor or the wall"""
    sc, tab, kept = cutref.card_scene()
    arr = sc.arrays()
    c = load(ctx, arr)
    c.set_material_cutouts(tab)
    o, d = scene_rays(sc, mode)
    p = aovs(c, S.aov_params(sc.getCamera(), W, H), mode, ("ids", "hit"))
    check_against_records(p, c.trace(T.ray_records(o, d), 0), arr)
    card = cutref.card_instances(arr)[0]
    on_card = p["ids"][..., 0] == card
    assert on_card.sum() > 100 and set(np.unique(p["ids"][on_card][:, 1])) <= set(int(k) for k in kept)
    plain = load(ctx, arr)  # no table: the whole card is there
    q = aovs(plain, S.aov_params(sc.getCamera(), W, H), mode, ("ids",))
    holes = (q["ids"][..., 0] == card) & ~on_card
    assert holes.sum() > 100 and set(np.unique(p["ids"][holes][:, 0])) <= {0, 1}  # the floor and the wall
    assert np.array_equal(p["ids"][~(q["ids"][..., 0] == card)], q["ids"][~(q["ids"][..., 0] == card)])


@pytest.mark.parametrize("mode", ["centre", "sample0"])
def test_blend_card_under_the_raw_rule(ctx, mode):
    """a blend card whose blocks have a = 0, 128 / 255 and 1: a hit counts iff a > 0"""
    alpha = np.array([[0, 128, 255, 0], [255, 0, 128, 255], [128, 255, 0, 128], [0, 128, 255, 255]], np.uint8)
    sc, cut, _ = cutref.card_scene(alpha=alpha)
    arr = sc.arrays()
    blend = np.zeros(len(cut), S.MATERIAL_BLEND)
    for f in ("opacity_texture", "opacity_channel", "opacity_scale", "opacity_bias"):
        blend[f] = cut[f]
    blend["active"] = (cut["threshold"] > 0).astype(np.uint32)
    c = load(ctx, arr)
    c.set_material_blend(blend)
    o, d = scene_rays(sc, mode)
    p = aovs(c, S.aov_params(sc.getCamera(), W, H), mode, ("ids", "hit"))
    check_against_records(p, c.trace(T.ray_records(o, d), 0), arr)
    _, blocks, _ = cutref.card_triangles()
    a_of_prim = np.array([alpha[by, bx] for by, bx in blocks])
    card = cutref.card_instances(arr)[0]
    seen = np.unique(p["ids"][p["ids"][..., 0] == card][:, 1])
    assert (a_of_prim[seen] > 0).all() and (a_of_prim[seen] == 128).any() and (a_of_prim[seen] == 255).any()
    plain = load(ctx, arr)
    q = aovs(plain, S.aov_params(sc.getCamera(), W, H), mode, ("ids",))
    gone = np.unique(q["ids"][(q["ids"][..., 0] == card) & (p["ids"][..., 0] != card)][:, 1])
    assert len(gone) > 0 and (a_of_prim[gone] == 0).all()


@pytest.mark.parametrize("mode", ["centre", "sample0"])
def test_light_proxy_is_kind_3(ctx, mode):
    """the room of cutref with the camera looking up at its rect light: kind 3, no material, P = o + t d, N = Ng = 0, facing 0, albedo 1"""
    sc, _, _ = cutref.card_scene(cards=False, eye=((0.2, 0.4, 1.5), (0.0, 3.0, 0.0), 50.0))
    arr = sc.arrays()
    c = load(ctx, arr)
    o, d = scene_rays(sc, mode)
    ap = S.aov_params(sc.getCamera(), W, H)
    p = aovs(c, ap, mode)
    rec = c.trace(T.ray_records(o, d), 0)
    check_against_records(p, rec, arr)
    check_against_records(p, T.oracle_for(arr).trace(T.ray_records(o, d), 0), arr)
    lit = p["ids"][..., 3].reshape(-1) == 3
    assert lit.sum() > 50 and (arr["instances"]["type"][p["ids"].reshape(-1, 4)[lit, 0]] == S.INSTANCE_LIGHT).all()
    assert (p["ids"].reshape(-1, 4)[lit, 2] == 0xFFFFFFFF).all()
    want = o[lit] + rec["t"][lit, None] * d[lit]  # float32: one rounded product, one rounded sum
    assert want.dtype == np.float32
    pos = p["position"].reshape(-1, 4)[lit]
    assert np.array_equal(bits(pos[:, :3]), bits(want)) and (pos[:, 3] == 1).all()
    for name in ("normal", "geom_normal", "texcoord"):
        assert (p[name].reshape(-1, 4)[lit] == 0).all(), name
    assert (p["albedo"].reshape(-1, 4)[lit] == 1).all()
    bound, want_d = aovref.depth_bound(ap["world_to_clip"], pos[:, :3])
    assert (np.abs(p["hit"].reshape(-1, 4)[lit, 3].astype(np.float64) - want_d) <= bound).all()
    miss = p["ids"][..., 3].reshape(-1) == 0
    for name in ("normal", "position", "geom_normal", "albedo", "texcoord"):
        assert (p[name].reshape(-1, 4)[miss] == 0).all(), name
    assert (p["hit"].reshape(-1, 4)[miss] == [-1, 0, 0, 1]).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3, 4: float64
# ---------------------------------------------------------------------------------------------------------------------------------------------
def float64_checks(c, name, mode):
    sc, arr, params, ap, texel, curves = scene_of(name)
    v = view_of(name, mode)
    o, d = rays_of(name, mode)
    p = aovs(c, ap, mode)
    flat = {k: a.reshape(-1, 4) for k, a in p.items()}
    kind = flat["ids"][:, 3]
    view = aovref.normals_view(p["normal"], p["ids"][..., 3])
    out = T.check_normals_view(lambda _: view, arr, params, texel, lambda o32, d32: c.trace(T.ray_records(o32, d32), 0), v)
    hit, sel = v["hit"], v["tri"]
    worst = {}
    if sel.any():
        assert (kind[sel] == 1).all()
        st = hitref.triangle_state(arr, hit)
        # POSITION: the bound test_position_and_geometric_normal uses, on the device's own value
        e = np.abs(flat["position"][:, :3].astype(np.float64) - st["position"]).max(axis=1)
        b = hitref.position_bound(st["scale"], hit["cos"])
        worst["position"] = float((e[sel] / b[sel]).max())
        assert (e[sel] <= b[sel]).all() and (flat["position"][sel, 3] == 1).all()
        # GEOM_NORMAL: direction_bound of a `blend` of length 1 without spread -- its 7 U cover the cross product of two edge differences (two differences, U of an edge
        # each; a component a b - c d: two products and a difference; 5 U of |e1| |e2|, and the scenes' edges meet at right angles: |e1 x e2| = |e1| |e2|)
        e = np.abs(flat["geom_normal"][:, :3].astype(np.float64) - st["geom_normal"]).max(axis=1)
        b = hitref.direction_bound(st["kappa"], 1.0, 0.0, 0.0, hit["cos"])
        worst["geom_normal"] = float((e[sel] / b[sel]).max())
        assert (e[sel] <= b[sel]).all() and (flat["geom_normal"][sel, 3] == 0).all()
        # facing
        front = (hit["dir"] * st["geom_normal"]).sum(1) < 0
        assert front[sel].any() and (flat["normal"][sel & front, 3] == 1).all() and (flat["normal"][sel & ~front, 3] == -1).all()
    # depth: float64 of the plane's own position, every pixel that hit
    hitp = kind != 0
    bound, want = aovref.depth_bound(ap["world_to_clip"], flat["position"][hitp, :3])
    e = np.abs(flat["hit"][hitp, 3].astype(np.float64) - want)
    worst["depth"] = float((e / bound).max())
    assert (e <= bound).all() and (flat["hit"][~hitp, 3] == 1).all()
    if v["curve"].any():
        cur = v["curve"]
        assert (kind[cur] == 2).all() and np.array_equal(bits(flat["geom_normal"][cur, :3]), bits(flat["normal"][cur, :3]))
        pt = o[cur].astype(np.float64) + flat["hit"][cur, 0:1].astype(np.float64) * d[cur].astype(np.float64)
        # a curve's position is origin + t direction carried to object space, moved into the cross-section of the curve at the INTERSECTOR's u and onto the radius there
        # (fill_curve's normal function does that to the point it is given, as the reference's: ps = c(u) + r unit((ps - c) - ((ps - c) . c') c' / |c'|^2)), and carried
        # back.  Two moves in object space: along the axis, by what the intersector's u is off the point's own -- it stops when its next step in u is shorter than
        # CURVE_DU and reports a point du |c'| further along the axis (hitref.curve_normal_bound) --, CURVE_DU speed; along the radius, by the point's distance from
        # the surface, below 1e-4 r (check_normals_view's bar, just asserted).  Both stretched by at most sigma_max on the way back.  The roundings: the point, 2 U L;
        # the difference with the translation and the 3 x 3 product with once-rounded inverse entries, 7 U, the 3 x 4 product back, 6 U, both at the other space's
        # scale, kappa L at most: 16 U kappa L covers them
        inst = int(flat["ids"][cur, 0][0])
        sv = np.linalg.svd(hitref.instance_matrix(arr, inst)[:, :3], compute_uv=False)
        scale = max(float(np.abs(pt).max()), float(np.abs(arr["instances"]["transform"]).max()))
        cs = hitref.curve_state(arr, inst, flat["ids"][cur, 1].astype(np.int64), pt)
        e = np.abs(flat["position"][cur, :3].astype(np.float64) - pt).max(axis=1)
        b = (hitref.CURVE_DU * cs["speed"] + 1e-4 * cs["radius"]) * sv[0] + 16 * hitref.U * scale * sv[0] / sv[-1]
        worst["curve_position"] = float((e / b).max())
        assert (e <= b).all()
    print(f"{name} {mode}: max error / bound -- " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()) + "; normals: " + ", ".join(f"{k} {x[-1]:.3f}" for k, x in out.items()))
    return worst


@pytest.mark.parametrize("name", list(T.SCENES))
def test_float64_sample_mode(ctx, name):
    float64_checks(load(ctx, scene_of(name)[1]), name, "sample0")


@pytest.mark.parametrize("name", [n for n in T.SCENES if n not in CENTRE_EXCLUDED])
def test_float64_pixel_centre_mode(ctx, name):
    assert len([n for n in T.SCENES if n not in CENTRE_EXCLUDED]) == 16
    float64_checks(load(ctx, scene_of(name)[1]), name, "centre")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5: albedo and texture coordinates
# ---------------------------------------------------------------------------------------------------------------------------------------------
def textured_quads():
    """tests/test_gpu_mtex.py's two quads: the left one PBR with a random 4 x 4 base-colour texture and a roughness map (channel g), uvs 0 ... 2 by 0 ... 1; the right
    one GLASS, untextured; the wall behind DIFFUSE"""
    from tests.test_gpu_mtex import two_quads

    tex = np.random.RandomState(9).randint(0, 256, (4, 4, 4)).astype(np.uint8)
    mats = [dict(type=S.MAT_PBR, base_color=(0.8, 0.5, 0.3), metallic=0.5, roughness=0.5, base_color_texture=1, roughness_texture=1, roughness_channel=1, roughness_scale=0.8,
                 roughness_bias=0.1), dict(type=S.MAT_GLASS, base_color=(0.9, 0.95, 1.0), ior=1.5)]
    return two_quads(0, 1, [tex], (0.0, 2.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0), materials=mats, distant=True)


def vertex_uvs(arr, inst, prim):
    """the unpacked uvs of the three vertices of triangles (inst, prim): (N, 3, 2) float32"""
    tinst, tprim, vid, _ = hitref.triangle_table(arr)
    key = {(int(i), int(p)): k for k, (i, p) in enumerate(zip(tinst, tprim))}
    rows = vid[[key[(int(i), int(p))] for i, p in zip(inst, prim)]]
    u, v = mtexref.unpack_uv(arr["vertices"]["uv"][rows])
    return np.stack([u, v], -1)


@pytest.mark.parametrize("mode", ["centre", "sample0"])
def test_albedo_and_texcoord(ctx, mode):
    sc, arr = textured_quads()
    assert "material_textures" in arr
    c = load(ctx, arr)
    p = {k: a.reshape(-1, 4) for k, a in aovs(c, S.aov_params(sc.getCamera(), W, H), mode).items()}
    tri = p["ids"][:, 3] == 1
    mat = p["ids"][:, 2]
    assert tri.mean() > 0.4 and {0, 1, 2} <= set(np.unique(mat[tri]))
    # ALBEDO is what the probe answers for (material, uv)
    probe = c.material_probe(mat[tri], p["texcoord"][tri, :2])
    assert np.array_equal(bits(p["albedo"][tri, :3]), bits(probe[:, :3])) and (p["albedo"][tri, 3] == 1).all()
    # ... the texture's on the mapped quad (it varies), the constant elsewhere
    on0 = tri & (mat == 0)
    assert len(np.unique(p["albedo"][on0, :3], axis=0)) > 50
    for m in (1, 2):
        assert (p["albedo"][tri & (mat == m), :3] == arr["materials"]["base_color"][m]).all()
    # TEXCOORD against the float64 blend of the unpacked vertex uvs at the HIT plane's barycentrics: 4 U of the largest |uv|
    uv3 = vertex_uvs(arr, p["ids"][tri, 0], p["ids"][tri, 1]).astype(np.float64)
    bu, bv = p["hit"][tri, 1].astype(np.float64), p["hit"][tri, 2].astype(np.float64)
    want = uv3[:, 0] * (1 - bu - bv)[:, None] + uv3[:, 1] * bu[:, None] + uv3[:, 2] * bv[:, None]
    err = np.abs(p["texcoord"][tri, :2].astype(np.float64) - want).max(axis=1)
    bound = 4 * hitref.U * np.abs(uv3).max(axis=(1, 2))
    print(f"texcoord {mode}: max error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all() and (p["texcoord"][tri, 2:] == 0).all() and np.ptp(p["texcoord"][on0, 0]) > 1.0


@pytest.mark.parametrize("name", ["curves-identity", "map-nonuniform-200-60-230", "flat-shear"])
def test_untextured_albedo_is_the_base_colour(ctx, name):
    """DIFFUSE and HAIR-on-curve (the curve scene), PBR with a normal map only (the map scene), DIFFUSE (flat)"""
    sc, arr, params, ap, texel, curves = scene_of(name)
    c = load(ctx, arr)
    p = {k: a.reshape(-1, 4) for k, a in aovs(c, ap, "centre", ("ids", "albedo", "texcoord")).items()}
    surf = (p["ids"][:, 3] == 1) | (p["ids"][:, 3] == 2)
    assert np.array_equal(p["albedo"][surf, :3], arr["materials"]["base_color"][p["ids"][surf, 2]]) and (p["albedo"][surf, 3] == 1).all()
    types = set(int(t) for t in arr["materials"]["type"][np.unique(p["ids"][surf, 2])])
    assert types == ({S.MAT_DIFFUSE, S.MAT_HAIR} if curves else ({S.MAT_PBR} if texel else {S.MAT_DIFFUSE}))
    assert (p["texcoord"][p["ids"][:, 3] == 2] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6: regions, bands, ragged sizes
# ---------------------------------------------------------------------------------------------------------------------------------------------
RW, RH = 37, 23  # 851 pixels: no multiple of 64
REGIONS = [None, (5, 3, 17, 11), (36, 22, 1, 1), (0, 22, 37, 1), (20, 0, 17, 23)]


def test_regions_bands_and_plane_subsets(ctx):
    sc, arr = textured_quads()
    ap = S.aov_params(sc.getCamera(), RW, RH)
    whole = None
    for band in (None, 64, 1000):  # 1000: bands that end mid-row, a ragged last band
        c = load(ctx, arr, RW, RH, **({} if band is None else {"aov_band": band}))
        full = aovs(c, ap, "sample0")
        if whole is None:
            whole = full
            assert len(np.unique(full["ids"][..., 3])) >= 2 and (full["ids"][..., 3] == 1).mean() > 0.4
        for k in ALL:
            assert np.array_equal(bits(full[k]), bits(whole[k])), (band, k)
        for reg in REGIONS[1:]:
            x0, y0, w, h = reg
            part = aovs(c, ap, "sample0", region=reg)
            for k in ALL:
                assert part[k].shape == (h, w, 4) and np.array_equal(bits(part[k]), bits(whole[k][y0:y0 + h, x0:x0 + w])), (band, reg, k)
        # a subset of planes writes the same bits and leaves the other buffers alone
        for subset in (("ids",), ("normal", "albedo")):
            import torch

            sentinel = np.full((RH, RW, 4), 0xDEADBEEF, np.uint32)
            bufs = [torch.full((RH, RW, 4), -559038737, dtype=torch.int32, device="cuda") for _ in ALL]  # 0xdeadbeef
            torch.cuda.synchronize()
            mask = sum(1 << ALL.index(k) for k in subset)
            p = np.array(ap)
            p["sample_index"], p["spp_total"] = 0, 64
            c.render_aovs_device(p, mask, [b.data_ptr() for b in bufs])  # (every pointer given: a clear bit must leave its buffer untouched)
            for k, b in zip(ALL, bufs):
                got = b.cpu().numpy().view(np.uint32)
                assert np.array_equal(got, bits(whole[k]) if k in subset else sentinel), (band, subset, k)
        # pick = the pixel of the planes
        for x, y in ((0, 0), (36, 22), (18, 11), (7, 20)):
            q = c.pick(S.aov_params(sc.getCamera(), RW, RH, sample_index=0, spp_total=64), x, y)
            for k in ALL:
                assert np.array_equal(bits(q[k]), bits(whole[k][y, x])), (x, y, k)


def test_bad_calls_are_refused_and_write_nothing(ctx):
    from strelka_amd import capi

    sc, arr = textured_quads()
    c = load(ctx, arr, RW, RH)
    ap = S.aov_params(sc.getCamera(), RW, RH)
    before = c.aov_info()
    with pytest.raises(capi.SkhError):
        c.render_aovs(ap, region=(30, 0, 8, 1))  # leaves the image
    with pytest.raises(capi.SkhError):
        c.render_aovs_device(ap, 0, [None] * 7)  # no plane
    with pytest.raises(capi.SkhError):
        c.render_aovs_device(ap, 1 << 7, [None] * 7)  # a bit above the last plane
    with pytest.raises(capi.SkhError):
        c.render_aovs_device(ap, 3, [None] * 7)  # a set bit without a buffer
    with pytest.raises(capi.SkhError):
        c.render_aovs(ap, sample_index=64, spp_total=64)
    assert c.aov_info() == before
    fresh = ctx()
    fresh.set_scene(arr)
    with pytest.raises(capi.SkhError, match="skh_resize"):
        fresh.render_aovs(ap)  # no image yet


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7: the frame is not disturbed
# ---------------------------------------------------------------------------------------------------------------------------------------------
CW, CH = 64, 48


def frame_state(c):
    return [c.read_accum(), c.read_aov(0), c.read_aov(1)]


@pytest.mark.parametrize("adaptive", [False, True])
def test_the_frame_is_not_disturbed(ctx, adaptive):
    sc = scenes.cornell_box()
    arr = sc.arrays()
    ap = S.aov_params(sc.getCamera(), CW, CH)
    a, b = load(ctx, arr, CW, CH), load(ctx, arr, CW, CH)
    for c in (a, b):
        if adaptive:
            c.set_adaptive(threshold=0.5, dark_level=0.05, min_samples=2, interval=1)
        c.reset_stats()
    sub = lambda c, i: c.render_subframe(S.frame_params(sc.getCamera(), CW, CH, subframe_index=i, spp_total=6, max_depth=4))
    for i in range(3):
        sub(a, i), sub(b, i)
    info = a.adaptive_info()
    planes = a.render_aovs(ap)
    assert a.adaptive_info() == info
    assert a.aov_info()["rays"] == CW * CH and a.aov_info()["calls"] == 1 and a.aov_info()["bytes_last"] == 7 * 16 * CW * CH and b.aov_info()["rays"] == 0
    for i in range(3, 6):
        sub(a, i), sub(b, i)
    for x, y in zip(frame_state(a), frame_state(b)):
        assert np.array_equal(bits(x), bits(y))
    if adaptive:
        assert np.array_equal(bits(a.read_adaptive()), bits(b.read_adaptive())) and a.adaptive_info() == b.adaptive_info()
        assert a.adaptive_info()["enabled"] == 1 and a.adaptive_info()["checks"] > 0
    sa, sb = a.stats(), b.stats()
    assert sa["rays_radiance"] == sb["rays_radiance"] > 0 and sa["rays_shadow"] == sb["rays_shadow"] > 0
    assert (planes["ids"][..., 3] == 1).mean() > 0.5
    # tile ownership is ignored: a context that owns every second tile answers for the whole image
    t = load(ctx, arr, CW, CH)
    tiles = [(x, y) for y in range(0, CH, 16) for x in range(0, CW, 16)][::2]
    t.set_tiles(16, tiles)
    sub(t, 0)
    q = t.render_aovs(ap)
    for k in ALL:
        assert np.array_equal(bits(q[k]), bits(planes[k])), k


def test_timing_spans_stay_out_of_the_trace_class(ctx):
    """with option timing, the pass's launches are a kernel class of their own: ms_trace_closest and launches_trace_closest do not move"""
    sc = scenes.cornell_box()
    c = load(ctx, sc.arrays(), CW, CH, timing=1)
    c.render_subframe(S.frame_params(sc.getCamera(), CW, CH, subframe_index=0, spp_total=4, max_depth=2))
    before = c.stats()
    c.render_aovs(S.aov_params(sc.getCamera(), CW, CH))
    after = c.stats()
    for k in ("ms_trace_closest", "ms_trace_shadow", "ms_shade", "ms_raygen", "launches_trace_closest", "launches_trace_shadow", "launches_shade", "launches_other"):
        assert after[k] == before[k], k
    assert c.aov_info()["ms_last"] > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8: oka::HipRender
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_hiprender_aovs_and_pick(tmp_path, ctx):
    """tests/cpp/hiprender_aov_main.cpp against the stand-in headers: renderAovs writes, byte for byte, the planes the ctypes path writes for the same scene and
    parameters; pick agrees with them at a mesh, a light and a miss pixel; the frame around the calls is the uninterrupted one"""
    import os
    import subprocess

    from strelka_amd import build
    from tests.test_host_cpp import load as load_dump, run_host

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, outd = tmp_path / "src", tmp_path / "aov"
    src.mkdir()
    outd.mkdir()
    run_host(src, "cpu")  # the scene of host_test.cpp as a .skscene dump
    build.build_host()
    exe = str(tmp_path / "hiprender_aov")
    host, lib = os.path.dirname(build.HOST_LIB), os.path.dirname(build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "cpp", "hiprender_aov_main.cpp"),
                           "-L" + host, "-loka_hip", "-L" + lib, "-lstrelka_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib])
    frames = 3
    out = subprocess.run([exe, str(outd), str(src / "scene.skscene"), str(frames)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [int(x) for x in open(outd / "frames.txt").read().split()] == [frames + 1, frames + 1]
    arr = load_dump(outd)
    w, h = 96, 64
    c = load(ctx, arr, w, h)
    ap = np.fromfile(outd / "aov_params.bin", S.AOV_PARAMS)[0]
    assert np.array_equal(ap["view_to_world"], arr["camera"][:16]) and np.array_equal(ap["clip_to_view"], arr["camera"][16:]) and int(ap["sample_index"]) == S.AOV_PIXEL_CENTRE
    v2w, c2v = (np.asarray(ap[k], np.float64).reshape(4, 4) for k in ("view_to_world", "clip_to_view"))
    assert np.abs(ap["world_to_clip"].reshape(4, 4) - np.linalg.inv(c2v) @ np.linalg.inv(v2w)).max() <= 2e-6 * np.abs(ap["world_to_clip"]).max()
    centre = c.render_aovs(ap)
    sample0 = c.render_aovs(ap, sample_index=0, spp_total=64)
    for k, name in enumerate(ALL):
        assert (outd / f"centre_{k}.bin").read_bytes() == centre[name].tobytes(), name
        assert (outd / f"sample0_{k}.bin").read_bytes() == sample0[name].tobytes(), name
    for k in (0, 2):
        assert (outd / f"region_{k}.bin").read_bytes() == np.ascontiguousarray(centre[ALL[k]][3:14, 5:22]).tobytes()
    picks = np.fromfile(outd / "picks.bin", np.uint32).reshape(-1, 30)
    kinds = [int(r[5]) for r in picks]
    assert kinds == sorted(set(int(k) for k in np.unique(centre["ids"][..., 3]))) and {0, 1, 3} <= set(kinds)  # a miss, the floor or the panel, a light's proxy
    for r in picks:
        x, y = int(r[0]), int(r[1])
        assert np.array_equal(r[2:], np.concatenate([bits(centre[name][y, x]) for name in ALL])), (x, y)
    # the frame: frames + 1 sub-frames as if never interrupted
    p = np.zeros((), S.FRAME_PARAMS)
    p["view_to_world"], p["clip_to_view"] = arr["camera"][:16], arr["camera"][16:]
    p["samples_this_launch"], p["spp_total"], p["max_depth"], p["enable_accumulation"] = 1, 64, 4, 1
    p["exposure"] = S.default_exposure()
    for i in range(frames + 1):
        p["subframe_index"] = i
        c.render_subframe(p)
    assert np.array_equal(c.read_accum(), np.fromfile(outd / "accum.bin", np.float32).reshape(h, w, 4))
