"""Cutouts restated on the CPU ("Cutouts") -- typed from the definition, not from the device code: the continuation is a Python loop
over the CPU checker's closest-hit query (a ray record carries its tmin: the loop needs nothing new), the opacity comes from tests/mtexref.py's look-up at
a uv interpolated in float64 from the unpacked vertex uvs, the accept / reject / round-limit rules are the definition's.

It is a reference for PLATEAU textures only: texel values 0 / 255 and a hit whose whole bilinear footprint -- widened by `margin` texels on every side -- lies
inside one plateau.  There the fp32 look-up gives exactly 0 or 1 and the fp32 and float64 decisions cannot differ.  `margin` is 1.5 for interpolated uvs (the
sample point then lies at least two texels from its plateau's border); for triangles whose three vertices carry ONE uv (a block centre: the footprint is the
block itself) the interpolated uv is that uv up to a few ulps and 0.25 covers it.
No ray is ever left out of a comparison: a footprint that leaves its plateau is an assertion failure, not a skipped ray.

The second half builds the scenes tests/test_cutout_cpu.py and tests/test_gpu_cutout.py share, and their ray grids."""
import math

import numpy as np

from strelka_amd import scene as S
from tests import mtexref

F = np.float32
HIT = np.dtype([("t", np.float32), ("instance_id", np.uint32), ("prim_id", np.uint32), ("u", np.float32), ("v", np.float32)])
NO_ID = 0xFFFFFFFF


def entry(**kw):
    e = np.zeros((), S.MATERIAL_CUTOUT)
    e["opacity_channel"], e["opacity_scale"] = 3, 1.0
    for k, v in kw.items():
        e[k] = v
    return e


def table(n, entries):
    """n materials, `entries` {material: entry(...)}"""
    t = np.zeros(n, S.MATERIAL_CUTOUT)
    t["opacity_channel"], t["opacity_scale"] = 3, 1.0
    for k, e in entries.items():
        t[k] = e
    return t


def footprint_is_plateau(tex, channel, uv, margin):
    """all texels the bilinear footprints of uv -/+ margin texels touch (wrap addressing) are equal in `channel`: -> (n,) bool"""
    tex = np.asarray(tex)
    h, w = tex.shape[:2]
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    x, y = (uv[:, 0] - np.floor(uv[:, 0])) * w - 0.5, (uv[:, 1] - np.floor(uv[:, 1])) * h - 0.5
    x0, x1 = np.floor(x - margin).astype(np.int64), np.floor(x + margin).astype(np.int64) + 1
    y0, y1 = np.floor(y - margin).astype(np.int64), np.floor(y + margin).astype(np.int64) + 1
    ok = np.ones(len(uv), bool)
    for k in range(len(uv)):
        xs, ys = np.arange(x0[k], x1[k] + 1) % w, np.arange(y0[k], y1[k] + 1) % h
        block = tex[np.ix_(ys, xs)][..., channel]
        ok[k] = (block == block.flat[0]).all() and block.flat[0] in (0, 255)
    return ok


def hit_uv(arr, inst, prim, bu, bv):
    """text_coords[0] of hits on mesh instances, in float64 from the unpacked vertex uvs: uv0 (1 - u - v) + uv1 u + uv2 v"""
    out = np.zeros((len(inst), 2))
    for k in range(len(inst)):
        me = arr["meshes"][int(arr["instances"][int(inst[k])]["geom_id"])]
        idx = arr["indices"][int(me["index_offset"]) + 3 * int(prim[k]):int(me["index_offset"]) + 3 * int(prim[k]) + 3].astype(np.int64) + int(me["vertex_offset"])
        u, v = mtexref.unpack_uv(arr["vertices"]["uv"][idx])
        w = np.array([1.0 - float(bu[k]) - float(bv[k]), float(bu[k]), float(bv[k])])
        out[k] = (np.asarray(u, np.float64) * w).sum(), (np.asarray(v, np.float64) * w).sum()
    return out


def opacity(e, textures, uv):
    """clamp01(fl(fl(scale * texel) + bias)), texel = 1 without a texture that exists: (n,) float32"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    tid = int(e["opacity_texture"])
    texel = np.ones(len(uv), F)
    if 0 < tid <= len(textures):
        texel = mtexref.lookup(textures[tid - 1], uv.astype(F))[:, int(e["opacity_channel"])]
    return mtexref.clamp01(((F(e["opacity_scale"]) * texel).astype(F) + F(e["opacity_bias"])).astype(F))


def trace(oracle, arr, cutouts, rays, mode=0, rounds=8, margin=0.25):
    """The definition over `oracle` (tests/orklib.Oracle with the scene set): -> (hits, info).  mode 0: HIT records of the nearest ACCEPTED hit; mode 1: t = 1
    (occluded: an accepted hit in (tmin, tmax]) or -1, the other fields as the product's shadow answers.  info: rays continued because their hit was cut away
    (per round), hits accepted by the round limit, whether a ray's FIRST hit was cut away."""
    textures = arr.get("textures") or []
    rays = np.array(rays, copy=True)
    n = len(rays)
    out = np.zeros(n, HIT)
    out["t"], out["instance_id"], out["prim_id"] = -1.0, NO_ID, NO_ID
    live = np.arange(n)
    info = {"continued": 0, "capped": 0, "first_cut": np.zeros(n, bool), "per_round": []}
    nmat = len(arr["materials"])
    for r in range(rounds + 1):
        if len(live) == 0:
            break
        last = r == rounds
        h = oracle.trace(rays[live], 0)
        again = []
        cont_here = 0
        for k, i in enumerate(live):
            inst = int(h["instance_id"][k])
            if inst == NO_ID:
                continue  # a miss: final (the record is a miss already)
            rec = arr["instances"][inst]
            typ = int(rec["type"])
            reject, proxy = False, False
            if typ == S.INSTANCE_LIGHT:
                proxy = mode == 1
            elif typ == S.INSTANCE_MESH:
                mid = int(rec["material_id"])
                mid = 0 if mid == NO_ID or mid >= nmat else mid
                e = cutouts[mid] if cutouts is not None and mid < len(cutouts) else None
                if e is not None and float(e["threshold"]) > 0.0:
                    uv = hit_uv(arr, [inst], [int(h["prim_id"][k])], [h["u"][k]], [h["v"][k]])
                    tid = int(e["opacity_texture"])
                    if 0 < tid <= len(textures):
                        assert footprint_is_plateau(textures[tid - 1], int(e["opacity_channel"]), uv, margin).all(), ("a hit leaves its plateau", i, uv)
                    reject = not bool(opacity(e, textures, uv)[0] >= F(e["threshold"]))
            if r == 0 and reject:
                info["first_cut"][i] = True
            if (reject or proxy) and not last:
                rays["tmin"][i] = h["t"][k]
                again.append(i)
                cont_here += 1 if reject else 0
                continue
            if reject and last:
                info["capped"] += 1
            if proxy:
                continue  # (met in the last round: a light proxy does not occlude)
            out[i] = h[k]
        info["continued"] += cont_here
        info["per_round"].append(cont_here)
        live = np.array(again, np.int64)
    if mode == 1:
        res = np.zeros(n, HIT)
        res["t"] = np.where(out["instance_id"] != NO_ID, F(1.0), F(-1.0))
        res["instance_id"], res["prim_id"] = NO_ID, NO_ID
        return res, info
    return out, info


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the scenes and ray grids the two test files share
# ---------------------------------------------------------------------------------------------------------------------------------------------
CARD_HALF, CARD_CELLS, CARD_Y = 0.8, 4, 1.0
CELL = 2 * CARD_HALF / CARD_CELLS


def block_alpha(seed=5, flip=False):
    """alpha (0 / 255) of the 4 x 4 blocks of the card's 8 x 8 texture: about half cut, never all or none"""
    a = np.random.RandomState(seed).randint(0, 2, (4, 4)).astype(np.uint8) * 255
    a[0, 0], a[3, 3] = 0, 255
    return 255 - a if flip else a


def card_texture(alpha):
    """8 x 8 RGBA8: colour noise (the colour is not looked at), alpha per 2 x 2 block"""
    t = np.random.RandomState(9).randint(0, 256, (8, 8, 4)).astype(np.uint8)
    t[..., 3] = np.kron(alpha, np.ones((2, 2), np.uint8))
    return t


def card_triangles():
    """the 32 triangles of the 4 x 4-cell card in its own frame (the plane y = 0, x and z in -/+ CARD_HALF), their block (by, bx) and block-centre uv"""
    tris, blocks = [], []
    for cz in range(CARD_CELLS):
        for cx in range(CARD_CELLS):
            x0, z0 = -CARD_HALF + cx * CELL, -CARD_HALF + cz * CELL
            a, b, c, d = (x0, 0.0, z0 + CELL), (x0 + CELL, 0.0, z0 + CELL), (x0 + CELL, 0.0, z0), (x0, 0.0, z0)
            tris += [(a, b, c), (a, c, d)]  # (wind towards +Y; the shared edge is the diagonal a-c: fx + fz = 1 in cell coordinates)
    for t in range(len(tris)):
        k = (5 * t + 3) % 16  # (the two triangles of a cell belong to different blocks)
        blocks.append((k // 4, k % 4))
    uv = np.array([((2 * bx + 1) / 8.0, (2 * by + 1) / 8.0) for by, bx in blocks])
    return np.float32(tris), blocks, uv


def card_mesh(sc, keep=None):
    """the card as a mesh of UNSHARED vertices, all three of a triangle with its block-centre uv; `keep`: (32,) bool, the triangles that stay (the twin)"""
    tris, _, uv = card_triangles()
    sel = np.arange(len(tris)) if keep is None else np.flatnonzero(keep)
    vb, ib = S.deindex(tris[sel].reshape(-1, 3), np.arange(3 * len(sel)).reshape(-1, 3))
    vb["uv"] = S.pack_uv(np.repeat(uv[sel], 3, axis=0).astype(np.float32))
    return sc.createMesh(vb, ib)


def card_kept(alpha):
    _, blocks, _ = card_triangles()
    return np.array([alpha[by, bx] == 255 for by, bx in blocks])


def quad_mesh(sc, p, uv=None):
    """two triangles over the corners p[0..3] (counter-clockwise seen from the front)"""
    t = np.float32([[p[0], p[1], p[2]], [p[0], p[2], p[3]]])
    vb, ib = S.deindex(t.reshape(-1, 3), np.arange(6).reshape(-1, 3))
    if uv is not None:
        vb["uv"] = S.pack_uv(np.float32([uv[0], uv[1], uv[2], uv[0], uv[2], uv[3]]))
    return sc.createMesh(vb, ib)


LIGHT_XF = S.translate((0.0, 3.0, 0.0)) @ S.rotate((1, 0, 0), math.radians(-90))  # a rect light that emits towards -Y


def room(sc, grey, light=True):
    """a floor quad, a wall behind, a rect light above"""
    sc.createInstance(S.INSTANCE_MESH, quad_mesh(sc, [(-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)]), grey, np.eye(4))
    sc.createInstance(S.INSTANCE_MESH, quad_mesh(sc, [(-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)]), grey, np.eye(4))
    if light:
        sc.createLight({"type": 0, "xform": LIGHT_XF, "useXform": True, "width": 1.5, "height": 1.5, "color": (10.0, 10.0, 10.0), "intensity": 1.0})


def camera(eye=(0.3, 2.2, 3.4), at=(0.0, 0.8, 0.0), fov=45.0):
    cam = S.Camera(fov=fov)
    cam.lookAt(eye, at)
    return cam


CARD_XFORMS = {"single": [S.translate((0.0, CARD_Y, 0.0))],
               # one mesh under two transforms, one of them mirrored (negative determinant): two cards side by side
               "shared": [S.translate((-0.9, CARD_Y, 0.2)) @ S.scale((0.5, 1.0, 0.5)), S.translate((0.9, 1.3, -0.1)) @ S.scale((-0.5, 1.0, 0.5))],
               # three parallel layers, the lowest first (a ray from above meets it third)
               "layers": [S.translate((0.0, 0.6, 0.0)), S.translate((0.0, 0.9, 0.0)), S.translate((0.0, 1.2, 0.0))],
               # upright in front of the hair stand-in's head, facing its camera
               "front": [S.translate((0.0, 0.3, 2.2)) @ S.rotate((1, 0, 0), math.radians(90))]}


def add_card(sc, mat, alpha, twin=False, xforms=None, layout="single"):
    """the card (or, `twin`, what is left of it) as one mesh under every transform of the layout -> the instance ids"""
    mesh = card_mesh(sc, card_kept(alpha) if twin else None)
    return [sc.createInstance(S.INSTANCE_MESH, mesh, mat, xf) for xf in (CARD_XFORMS[layout] if xforms is None else xforms)]


def card_scene(twin=False, layout="single", alpha=None, extra=None, cut_slot=1, light=True, eye=None, xforms=None, cards=True):
    """-> (scene, cutout table or None, kept-triangle map).  Materials: 0 grey, `cut_slot` the card's (base colour from its texture's rgb);
    the twin has the cut triangles deleted and no table.  `extra(sc)` adds more to both alike; `cards` False: the room alone (same materials and textures)."""
    alpha = block_alpha() if alpha is None else alpha
    sc = S.Scene()
    tex = sc.addTexture(card_texture(alpha))
    n = max(2, cut_slot + 1)
    for k in range(n):
        sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6), base_color_texture=tex if k == cut_slot else 0)
    room(sc, 0, light)
    keep = card_kept(alpha)
    if cards and not (twin and not keep.any()):  # (the twin of a fully cut card has no card at all)
        add_card(sc, cut_slot, alpha, twin, xforms, layout)
    if extra is not None:
        extra(sc)
    sc.addCamera(camera() if eye is None else camera(*eye))
    tab = None if twin else table(n, {cut_slot: entry(opacity_texture=tex, opacity_channel=3, threshold=0.5)})
    return sc, tab, np.flatnonzero(keep)


def card_instances(arr, first=2):
    """ids of the card instances of card_scene (behind the floor and the wall; the light's proxy follows them)"""
    return [k for k in range(first, len(arr["instances"])) if int(arr["instances"][k]["type"]) == S.INSTANCE_MESH]


def grid_targets(n=64):
    """n x n points of the card's own frame, clear of the cell edges and of the cells' diagonals by construction: cell-local (fx, fz) =
    ((i + 0.37) / 16, (j + 0.31) / 16) mod 1 -- at least 0.019 from 0 and 1, fx + fz at least 0.02 from 1"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x = -CARD_HALF + 2 * CARD_HALF * (i + 0.37) / n
    z = -CARD_HALF + 2 * CARD_HALF * (j + 0.31) / n
    return np.stack([x.reshape(-1), np.zeros(n * n), z.reshape(-1)], -1)


def make_rays(origins, targets, tmax=1e16):
    r = np.zeros(len(targets), S.RAY)
    o = np.broadcast_to(np.asarray(origins, np.float64), targets.shape)
    d = targets - o
    r["origin"], r["dir"] = o, d / np.linalg.norm(d, axis=1, keepdims=True)
    r["tmin"], r["tmax"] = 0.0, tmax
    return r


def card_rays(layout="single", oblique=False, count=4096):
    """rays through the cards of CARD_XFORMS[layout]: straight down (along the card's own -Y) from above every target, or oblique from one point per card;
    `count` of the 4096 x cards, evenly spread.  The layers share one set of rays: through all three."""
    out = []
    for xf in CARD_XFORMS[layout][-1:] if layout == "layers" else CARD_XFORMS[layout]:
        tg = (np.c_[grid_targets(), np.ones(4096)] @ xf.T)[:, :3]
        if oblique:
            out.append(make_rays((xf @ np.array([0.35, 1.6, 0.45, 1.0]))[:3], tg))
        else:
            out.append(make_rays(tg + xf[:3, 1] * 1.5, tg))
    r = np.concatenate(out)
    return r[np.linspace(0, len(r) - 1, count).astype(np.int64)] if count < len(r) else r


def shadow_version(rays):
    """the same rays as shadow rays: every second one ends between the card and the floor, the others reach the floor"""
    r = np.array(rays, copy=True)
    r["tmax"] = np.where(np.arange(len(r)) % 2 == 0, 1.9, 6.0).astype(np.float32)
    return r


def edge_clearance(rays, layout="single"):
    """for every ray the distance (in cell units) of its crossing of each card's plane from the nearest cell edge or cell diagonal, over the cards it crosses
    inside their extent; inf for a ray that crosses none: computed in float64 from the ray records"""
    o, d = np.asarray(rays["origin"], np.float64), np.asarray(rays["dir"], np.float64)
    best = np.full(len(rays), np.inf)
    for xf in CARD_XFORMS[layout]:
        inv = np.linalg.inv(xf)
        ol, dl = (np.c_[o, np.ones(len(o))] @ inv.T)[:, :3], d @ inv[:3, :3].T
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -ol[:, 1] / dl[:, 1]
        p = ol + t[:, None] * dl
        inside = (t > 0) & (np.abs(p[:, 0]) < CARD_HALF) & (np.abs(p[:, 2]) < CARD_HALF)
        fx, fz = ((p[:, 0] + CARD_HALF) / CELL) % 1.0, ((p[:, 2] + CARD_HALF) / CELL) % 1.0
        c = np.minimum.reduce([fx, 1 - fx, fz, 1 - fz, np.abs(fx + fz - 1.0) / math.sqrt(2.0)])
        # (a crossing just outside the card's border counts with its distance from the border)
        border = np.maximum(np.abs(p[:, 0]), np.abs(p[:, 2])) / CELL - CARD_HALF / CELL
        c = np.where(inside, c, np.where(t > 0, np.abs(border), np.inf))
        best = np.minimum(best, c)
    return best


# the interpolated-uv object: one quad with uv 0..1 and a 16 x 4 texture, left half alpha 0 / red 0, right half 255
def half_texture():
    t = np.zeros((4, 16, 4), np.uint8)
    t[:, 8:, 3], t[:, 8:, 0] = 255, 255
    t[..., 1] = 77
    return t


def half_scene():
    """a 2 x 1 quad at height 1 over the floor, u along x over 0..1, v along z -> (scene, texture id)"""
    sc = S.Scene()
    tex = sc.addTexture(half_texture())
    sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    sc.addMaterial(S.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    room(sc, 0)
    sc.createInstance(S.INSTANCE_MESH, quad_mesh(sc, [(-1, 1, 0.5), (1, 1, 0.5), (1, 1, -0.5), (-1, 1, -0.5)], [(0, 1), (1, 1), (1, 0), (0, 0)]), 1, np.eye(4))
    sc.addCamera(camera())
    return sc, tex


def half_rays(n=24):
    """rays aimed at u in [0.15, 0.35] and [0.65, 0.85] of the quad of half_scene (clear of the border at 0.5 and of the wrap), v over (0.1, 0.9): straight down and oblique"""
    u = np.concatenate([np.linspace(0.15, 0.35, n), np.linspace(0.65, 0.85, n)])
    v = 0.1 + 0.8 * ((np.arange(2 * n) * 7 + 3) % 16) / 16.0
    tg = np.stack([2 * u - 1, np.ones(2 * n), v - 0.5], -1)
    return np.concatenate([make_rays(tg + np.array([0.0, 1.0, 0.0]), tg), make_rays((0.2, 2.6, 0.9), tg)]), np.concatenate([u, u])
