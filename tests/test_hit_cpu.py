"""Hit reconstruction of the CPU checker (oracle/oracle.cpp: fill_triangle, fill_curve, xform_normal, xform_point, invert_affine) against the float64
restatement in tests/hitref.py, under instance transforms that tell M from inverse(M)^T, a direction from a point, one vertex from another and one side
from the other.  The observable is the `debug = 1` view, (state.normal + 1) / 2 of the first hit, and -- for position and geometric normal -- the origins of
the rays that leave the first hit, from the checker's path log.  Every bar is a function of tests/hitref.py with its derivation; every scene's hit share and
excluded share are asserted from the reference alone.  tests/test_gpu_hit.py runs the same scenes and the same check_normals_view on the device."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from tests import hitref, orklib

W, H = 96, 72
FOV = 35.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# transforms
# ---------------------------------------------------------------------------------------------------------------------------------------------
def random_rotation(seed):
    q = np.random.RandomState(seed).normal(size=4)
    return S.quat_to_mat4(q / np.linalg.norm(q))


def shear():
    m = np.eye(4)
    m[0, 1], m[0, 2], m[1, 2] = 0.6, 0.3, 0.4
    return m


TRANSFORMS = {
    "identity": np.eye(4),
    "rotation": random_rotation(11),
    "uniform3": S.scale((3.0, 3.0, 3.0)),
    "nonuniform": random_rotation(12) @ S.scale((2.0, 1.0, 0.25)),
    "shear": shear(),
    "mirror": random_rotation(13) @ S.scale((-1.0, 1.0, 1.0)),
    "far": S.translate((4096.0, 0.0, 0.0)) @ random_rotation(14),
    "kappa16": S.scale((8.0, 1.0, 0.5)),
}
CURVE_TRANSFORMS = {"identity": np.eye(4), "nonuniform": random_rotation(15) @ S.scale((2.0, 1.0, 0.5))}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes: a few large triangles that fill most of the frame, seen from the side their (transformed) normals point to, a rect light behind the camera
# ---------------------------------------------------------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def quad_vertices(centre, ex, ey, normals=None, tangents=None):
    """corners centre -+ ex -+ ey, counter-clockwise seen from ex x ey; face normal and ex as normal / tangent unless given"""
    c, ex, ey = (np.asarray(a, np.float64) for a in (centre, ex, ey))
    pos = np.stack([c - ex - ey, c + ex - ey, c + ex + ey, c - ex + ey])
    n = np.tile(unit(np.cross(ex, ey)), (4, 1)) if normals is None else unit(normals)
    t = np.tile(unit(ex), (4, 1)) if tangents is None else unit(tangents)
    return S.make_vertices(pos, n, [(0, 0), (1, 0), (1, 1), (0, 1)], t), pos


FACES = (0, 1, 2, 2, 3, 0)  # two triangles that share the diagonal 0-2 and name it in different vertex orders


def place_camera(sc, M, pts_obj, n_obj, mode, fill, target_obj=None):
    """eye on the side inverse(M3)^T n_obj points to, up = the image of the object's y axis, looking at the image of target_obj (default: the middle of the
    transformed points' bounding rectangle); the distance puts the frame inside (`mode` "inside") or around ("around") that rectangle, times `fill`.  The rect
    light sits behind the camera and shines along the view."""
    M = np.asarray(M, np.float64)
    M3 = M[:3, :3]
    pw = np.asarray(pts_obj, np.float64) @ M3.T + M[:3, 3]
    nw = unit(np.linalg.inv(M3).T @ np.asarray(n_obj, np.float64))
    up = unit(M3 @ np.array([0.0, 1.0, 0.0]))
    s = unit(np.cross(-nw, up))
    u = np.cross(s, -nw)
    a, b, dpt = pw @ s, pw @ u, pw @ nw
    at, bt = ((a.max() + a.min()) / 2, (b.max() + b.min()) / 2) if target_obj is None else ((M3 @ np.asarray(target_obj, np.float64) + M[:3, 3]) @ v for v in (s, u))
    cw = s * at + u * bt + nw * dpt.max()
    side = min if mode == "inside" else max
    ex, ey = side(a.max() - at, at - a.min()), side(b.max() - bt, bt - b.min())
    ty = math.tan(math.radians(FOV) / 2)
    tx = ty * W / H
    pick = min if mode == "inside" else max
    D = fill * pick(ex / tx, ey / ty)
    eye = cw + D * nw
    cam = S.Camera(fov=FOV)
    cam.lookAt(eye, cw, up)
    sc.addCamera(cam)
    xf = np.eye(4)
    xf[:3, 0], xf[:3, 1], xf[:3, 2], xf[:3, 3] = s, u, nw, eye + 0.5 * D * nw  # the light emits towards its local -Z
    sc.createLight({"type": 0, "xform": xf, "useXform": True, "width": D, "height": D, "color": (1.0, 1.0, 1.0), "intensity": 20.0})
    return D


def flat_scene(name):
    """three quads whose vertex normals are their face normals, each an instance of its own mesh under TRANSFORMS[name]: one to the left tilted about y, one in
    the middle and one above it tilted about x -- an L, so that a transform that stretches one axis still leaves two of them in the frame"""
    M = TRANSFORMS[name]
    sc = S.Scene()
    mat = sc.addMaterial(S.MAT_DIFFUSE, (0.7, 0.6, 0.5))
    c25, s25, c15, s15 = math.cos(math.radians(25)), math.sin(math.radians(25)), math.cos(math.radians(15)), math.sin(math.radians(15))
    pts = []
    for centre, ex, ey in (((-2.1, 0.0, 0.3), (c25, 0, -s25), (0, 1, 0)), ((0.0, 0.0, 0.0), (1, 0, 0), (0, c15, s15)), ((0.0, 2.1, 0.2), (1, 0, 0), (0, c25, -s25))):
        vb, pos = quad_vertices(centre, 0.95 * np.asarray(ex), 0.95 * np.asarray(ey))
        sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, FACES), mat, M)
        pts.append(pos)
    place_camera(sc, M, np.concatenate(pts), (0, 0, 1), "inside", 0.8, target_obj=(-0.5, 0.6, 0.0))
    return sc


SMOOTH_NORMALS = [(-0.4, -0.3, 1.0), (0.5, -0.2, 1.0), (0.3, 0.5, 1.0), (-0.45, 0.35, 1.0)]  # 26 ... 30 degrees off the face normal +z
SMOOTH_TANGENTS = [(1.0, 0.2, 0.4), (1.0, -0.3, -0.5), (1.0, 0.25, -0.3), (1.0, -0.1, 0.45)]


def smooth_quad(normals=SMOOTH_NORMALS):
    return quad_vertices((0, 0, 0), (1.2, 0, 0), (0, 1.2, 0), normals, SMOOTH_TANGENTS)


def smooth_scene(name, texel=None, normals=SMOOTH_NORMALS):
    """one quad of two triangles with four different vertex normals (and tangents); with `texel` a constant 4 x 4 normal map of that colour"""
    M = TRANSFORMS[name]
    sc = S.Scene()
    if texel is None:
        mat = sc.addMaterial(S.MAT_DIFFUSE, (0.7, 0.6, 0.5))
    else:
        tex = np.zeros((4, 4, 4), np.uint8)
        tex[...] = tuple(texel) + (255,)
        mat = sc.addMaterial(S.MAT_PBR, (0.7, 0.6, 0.5), roughness=0.6, metallic=0.0, normal_texture=sc.addTexture(tex))
    vb, pos = smooth_quad(normals)
    sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, FACES), mat, M)
    place_camera(sc, M, pos, (0, 0, 1), "around", 1.1)
    return sc


TILTED = unit(math.sin(math.radians(30)) * np.array([0.6, 0.8, 0.0]) + math.cos(math.radians(30)) * np.array([0.0, 0.0, 1.0]))


def tilted_scene(name):
    """a flat quad whose four vertex normals are one direction 30 degrees off its face normal"""
    return smooth_scene(name, normals=[TILTED] * 4)


def shared_scene():
    """ONE mesh (the smooth quad), three instances: as it is, under a non-uniform scale, mirrored.  (Rotations about z only: all three face the camera.)"""
    sc = S.Scene()
    mat = sc.addMaterial(S.MAT_DIFFUSE, (0.7, 0.6, 0.5))
    vb, pos = smooth_quad()
    mesh = sc.createMesh(vb, FACES)
    xfs = [S.translate((-1.4, 1.4, 0.0)), S.translate((0.0, -1.3, 0.1)) @ S.rotate((0, 0, 1), math.radians(8)) @ S.scale((2.2, 1.0, 0.5)),
           S.translate((1.4, 1.4, -0.1)) @ S.rotate((0, 0, 1), math.radians(-6)) @ S.scale((-1.0, 1.0, 1.0))]
    world = []
    for xf in xfs:
        sc.createInstance(S.INSTANCE_MESH, mesh, mat, xf)
        world.append(pos @ xf[:3, :3].T + xf[:3, 3])
    place_camera(sc, np.eye(4), np.concatenate(world), (0, 0, 1), "around", 1.0)
    return sc


def curve_scene(name):
    """two thick strands in front of a flat backdrop, all under CURVE_TRANSFORMS[name]: strand 0 of constant radius 0.12, strand 1 tapering from 0.15 to 0.08
    (r' != 0 everywhere); both leave the frame on either side, so no end cap is seen"""
    M = CURVE_TRANSFORMS[name]
    sc = S.Scene()
    mat = sc.addMaterial(S.MAT_DIFFUSE, (0.7, 0.6, 0.5))
    hair = sc.addHairMaterial((0.35, 0.2, 0.1), roughness_r=0.3, roughness_n=0.3)
    vb, pos = quad_vertices((0, 0, -0.6), (2.0, 0, 0), (0, 1.2, 0))
    sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, FACES), mat, M)
    k = np.arange(9)
    x = -2.4 + 0.6 * k
    strands = [np.stack([x, 0.42 + 0.08 * np.sin(1.1 * k), 0.1 * np.cos(1.3 * k)], 1), np.stack([x, -0.42 + 0.07 * np.cos(0.9 * k), 0.08 * np.sin(1.7 * k)], 1)]
    radii = [np.full(9, 0.12), np.linspace(0.15, 0.08, 9)]
    P, R = [], []
    for p, r in zip(strands, radii):  # phantom points at both ends, as the reference's BasisCurves adapter adds them
        P.append(np.concatenate([2 * p[:1] - p[1:2], p, 2 * p[-1:] - p[-2:-1]]))
        R.append(np.concatenate([r[:1], r, r[-1:]]))
    cid = sc.createCurve([11, 11], np.concatenate(P), np.concatenate(R))
    sc.createInstance(S.INSTANCE_CURVE, cid, hair, M)
    D = place_camera(sc, M, pos, (0, 0, 1), "inside", 0.75)
    assert D <= 4.0
    return sc


# every scene of this file by name: (builder, the normal map's texel or None, has curves); tests/test_gpu_hit.py runs them all on the device
SCENES = {**{f"flat-{n}": (functools.partial(flat_scene, n), None, False) for n in TRANSFORMS},
          **{f"smooth-{n}": (functools.partial(smooth_scene, n), None, False) for n in ("nonuniform", "mirror")},
          "shared": (shared_scene, None, False),
          **{f"tilted-{n}": (functools.partial(tilted_scene, n), None, False) for n in ("identity", "nonuniform")},
          **{f"map-{n}-{'-'.join(map(str, t))}": (functools.partial(smooth_scene, n, t), t, False) for n in ("nonuniform", "mirror") for t in ((255, 128, 128), (128, 255, 128), (200, 60, 230))},
          **{f"curves-{n}": (functools.partial(curve_scene, n), None, True) for n in CURVE_TRANSFORMS}}


def debug_params(sc, **kw):
    kw = {"subframe_index": 0, "spp_total": 64, "max_depth": 4, "debug": 1, "enable_accumulation": 0, **kw}
    return S.frame_params(sc.getCamera(), W, H, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the reference's view of a scene: before any renderer is looked at
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jitter():
    j = hitref.sampler_jitter(W, H, 0, spp_total=64, seed=52)
    j.setflags(write=False)
    return j


def reference_view(arr, params):
    """rays, float64 hits, and the classes of pixels: `tri` (a triangle is hit for certain), `curve` (a strand is), `miss` (nothing is), `excluded` (the rest)"""
    rays = hitref.camera_rays(params, W, H, 0, jitter())
    hit = hitref.first_hits(arr, rays)
    clr, cinst, cwhere = hitref.curve_clearance(arr, rays)
    found = hit["inst"] >= 0
    curve_unclear = np.abs(clr) <= hitref.CURVE_EDGE
    curve = clr < -hitref.CURVE_EDGE
    assert (~curve | ~found | (cwhere < hit["t"])).all()  # (the scenes keep their strands in front of their triangles)
    hits_any = found | (clr < 0)
    excluded = hit["unclear"] | curve_unclear
    v = {"rays": rays, "hit": hit, "curve": curve & ~excluded, "curve_instance": cinst, "tri": found & ~curve & ~excluded, "miss": ~found & ~(clr < 0) & ~excluded,
         "excluded": excluded, "hits_any": hits_any}
    share, lost = hits_any.mean(), excluded.sum() / max(1, hits_any.sum())
    print(f"reference: {share:.1%} of the frame hits something ({int(v['tri'].sum())} triangle, {int(v['curve'].sum())} curve pixels), {lost:.2%} of that excluded")
    assert share >= 0.40 and lost <= 0.01
    return v


def check_normals_view(render, arr, params, texel=None, trace=None, view=None):
    """`render(params)` -> the (H, W, >= 3) float32 `debug = 1` image of the scene `arr`; `trace(origin, direction)` -> the renderer's hit records (t, instance_id,
    prim_id, u, v) of those float32 rays.  2 image - 1 is held per pixel against hitref.triangle_state / hitref.curve_state under the derived bounds; pixels the
    reference says miss must be black.  Triangles are judged twice: at hitref's own float64 barycentrics, under a bound that carries the fp32 intersector's
    barycentric error, and at the renderer's fp32 barycentrics -- which must lie within that error of hitref's, on hitref's triangle -- as INPUTS of the blend, under
    the roundings of reconstruction alone.  A curve's t and segment are inputs of its normal likewise.  `view`: reference_view(arr, params), for a caller that
    checks several renderers of one scene.  -> the figures, for the record."""
    v = reference_view(arr, params) if view is None else view
    img = np.asarray(render(params), np.float32)[..., :3].reshape(-1, 3)
    got = 2.0 * img.astype(np.float64) - 1.0
    out = {}
    assert v["miss"].sum() == 0 or (img[v["miss"]] == 0).all()
    hit = v["hit"]
    o32, d32 = (a.reshape(-1, 3) for a in v["rays"])
    rec = trace(o32, d32)
    assert (rec["instance_id"][v["miss"]] == 0xFFFFFFFF).all()
    sel = v["tri"]
    if sel.any():
        assert (hit["cos"][sel] >= 0.5).all()  # incidence within 60 degrees of the normal
        assert np.array_equal(rec["instance_id"][sel], hit["inst"][sel]) and np.array_equal(rec["prim_id"][sel], hit["prim"][sel])
        st = hitref.triangle_state(arr, hit, texel)
        e_b = hitref.barycentric_error(st["size_ratio"], hit["cos"])
        bary32 = np.stack([rec["u"], rec["v"]], 1).astype(np.float64)
        db = np.abs(bary32 - hit["bary"]).max(axis=1)
        out["bary"] = (float(db[sel].max()), float((db[sel] / e_b[sel]).max()))
        assert (db[sel] <= e_b[sel]).all()
        for key, h, ratio in (("tri", hit, st["size_ratio"]), ("tri_fp32_bary", {**hit, "bary": bary32}, 0.0)):
            s2 = st if h is hit else hitref.triangle_state(arr, h, texel)
            e_n = hitref.direction_bound(s2["kappa"], s2["n_len"], s2["n_spread"], ratio, hit["cos"])
            if texel is None:
                want, bound = s2["normal"], e_n
            else:
                e_t = hitref.direction_bound(s2["kappa"], s2["t_len"], s2["t_spread"], ratio, hit["cos"])
                want, bound = s2["mapped"], hitref.mapped_bound(e_n, e_t, s2["ts"], s2["m_len"])
            err = np.abs(got - want).max(axis=1)
            out[key] = (float(err[sel].max()), float(bound[sel].max()), float((err[sel] / bound[sel]).max()))
            print(f"{key}: {int(sel.sum())} pixels, max |dn| {out[key][0]:.3e} = {out[key][0] / hitref.U:.1f} U, bound up to {out[key][1]:.3e} = {out[key][1] / hitref.U:.0f} U, "
                  f"max error / bound {out[key][2]:.3f}")
            assert (err[sel] <= bound[sel]).all()
        print(f"barycentrics: max |fp32 - float64| {out['bary'][0]:.3e}, max error / bound {out['bary'][1]:.3f}")
    sel = v["curve"]
    if sel.any() or (arr["instances"]["type"] == 2).any():
        is_curve = np.isin(rec["instance_id"], np.nonzero(arr["instances"]["type"] == 2)[0])
        assert is_curve[sel].all() and not is_curve[v["tri"] | v["miss"]].any()
        caps = sel & ((rec["u"] == 0.0) | (rec["u"] == 1.0))  # the end caps have a rule of their own
        lost = (v["excluded"].sum() + caps.sum()) / max(1, v["hits_any"].sum())
        assert lost <= 0.01
        sel = sel & ~caps
        idx = np.nonzero(sel)[0]
        inst = int(v["curve_instance"][idx[0]])
        assert (rec["instance_id"][idx] == inst).all()
        p = o32[idx].astype(np.float64) + rec["t"][idx].astype(np.float64)[:, None] * d32[idx].astype(np.float64)
        cs = hitref.curve_state(arr, inst, rec["prim_id"][idx], p)
        assert (cs["residual"] <= 1e-4 * cs["radius"]).all(), float((cs["residual"] / cs["radius"]).max())
        bound = hitref.curve_normal_bound(cs["scale"], cs["radius"], cs["kappa"], cs["bend"], cs["speed"])
        err = np.abs(got[idx] - cs["normal"]).max(axis=1)
        for k, name in enumerate(("constant", "tapering")):
            m = rec["prim_id"][idx] // 8 == k
            assert m.sum() > 200
            out["curve_" + name] = (float(err[m].max()), float(bound[m].max()), float((err[m] / bound[m]).max()))
            print(f"{name} strand: {int(m.sum())} pixels, max |dn| {err[m].max():.3e}, bound up to {bound[m].max():.3e}, max error / bound {(err[m] / bound[m]).max():.3f}; "
                  f"surface residual / r up to {(cs['residual'][m] / cs['radius'][m]).max():.2e}")
        assert (err <= bound).all()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the checker as the renderer
# ---------------------------------------------------------------------------------------------------------------------------------------------
def oracle_for(arr, bake=None):
    o = orklib.new_context()
    if bake is not None:
        o.set_bake(bake)
    o.set_scene(arr)
    o.resize(W, H)
    return o


def oracle_render(o):
    def render(params):
        o.render_subframe(params)
        return o.read_image()

    return render


def ray_records(o32, d32):
    rays = np.zeros(len(o32), orklib.RAY_DTYPE)
    rays["origin"], rays["dir"], rays["tmax"] = o32, d32, 1e16
    return rays


def oracle_trace(o, params):
    """t, instance and primitive from ray 0 of the checker's path log, pixel by pixel; u from its trace() of the same rays, which must name the same hit"""

    def trace(o32, d32):
        rec = o.trace(ray_records(o32, d32), 0)
        for i in range(len(o32)):
            rows, _ = o.debug_path(params, i % W, i // W, 0)
            r = rows[0]
            assert r[0] == 0 and np.array_equal(r[1:4], o32[i]) and np.array_equal(r[5:8], d32[i])
            assert (r[9] == rec["t"][i] and int(r[10]) == rec["instance_id"][i] and int(r[11]) == rec["prim_id"][i]) if r[9] >= 0 else rec["instance_id"][i] == 0xFFFFFFFF
        return rec

    return trace


def run_cpu(sc, texel=None, curves=False, bake=None):
    arr = sc.arrays()
    o = oracle_for(arr, bake)
    params = debug_params(sc)
    return check_normals_view(oracle_render(o), arr, params, texel, oracle_trace(o, params) if curves else lambda o32, d32: o.trace(ray_records(o32, d32), 0))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the reference checks itself
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_rays_are_the_ones_the_checker_traces():
    sc = flat_scene("rotation")
    arr, params = sc.arrays(), debug_params(sc)
    o = oracle_for(arr)
    ro, rd = hitref.camera_rays(params, W, H, 0, jitter())
    for px, py in ((0, 0), (95, 71), (17, 40), (48, 36), (80, 3), (3, 66)):
        rows, _ = o.debug_path(params, px, py, 0)
        assert np.array_equal(rows[0][1:4].view(np.uint32), ro[py, px].view(np.uint32)) and np.array_equal(rows[0][5:8].view(np.uint32), rd[py, px].view(np.uint32))
    assert 0 <= jitter().min() and jitter().max() < 1 and np.ptp(jitter()) > 0.9


def test_first_hits_solve_the_ray_equation():
    """origin + t direction = p0 w + p1 u + p2 v in world space, to float64's precision; unpack_normal is the exact q / 256 - 1"""
    sc = shared_scene()
    arr, params = sc.arrays(), debug_params(sc)
    hit = hitref.first_hits(arr, hitref.camera_rays(params, W, H, 0, jitter()))
    ok = hit["inst"] >= 0
    st = hitref.triangle_state(arr, hit)
    p = hit["origin"] + hit["t"][:, None] * hit["dir"]
    assert ok.mean() > 0.4 and np.abs(p[ok] - st["position"][ok]).max() < 1e-12 and (hit["min_bary"][ok] >= 0).all()
    assert len(np.unique(hit["inst"][ok])) == 3 and set(np.unique(hit["prim"][ok])) == {0, 1}
    n = hitref.unpack_normal(np.uint32([0, 0x3FF | (0x200 << 10) | (0x100 << 20), 0xFFFFFFFF]))
    assert np.array_equal(n, [[-1, -1, -1], [1023 / 256 - 1, 1.0, 0.0], [1023 / 256 - 1, 1023 / 256 - 1, 4095 / 256 - 1]])


def test_curve_state_against_finite_differences_and_a_cone():
    """hitref.curve_state on points built ON the surface, x = c(u) + r(u) e with e perpendicular to c'(u): it returns u, a zero residual, and the direction of the
    cross product of the surface's two partial derivatives, taken by central differences of that very parametrisation (e = the normalised part of a fixed vector
    w perpendicular to c'(u): d/du at fixed w, and the rotation about the axis).  On a straight strand whose radius grows linearly -- a cone -- the normal
    leans against the axis by atan(r' / |c'|), elementary geometry."""
    sc = curve_scene("identity")
    arr = sc.arrays()
    inst = int(np.nonzero(arr["instances"]["type"] == 2)[0][0])
    rs = np.random.RandomState(3)
    n = 400
    seg, u, w = rs.randint(0, 16, n), rs.uniform(0.02, 0.98, n), rs.normal(size=(n, 3))
    q = hitref.segment_control_points(arr, inst, seg)

    def surface(uu):
        c0, c1 = hitref.bspline(q, uu), hitref.bspline(q, uu, 1)
        t = unit(c1[:, :3])
        e = unit(w - (w * t).sum(1)[:, None] * t)
        return c0[:, :3] + c0[:, 3:4] * e, t, e, c0, c1

    x, t, e, c0, c1 = surface(u)
    h = 1e-6
    du = (surface(u + h)[0] - surface(u - h)[0]) / (2 * h)
    dphi = np.cross(t, e)
    want = unit(np.cross(dphi, du))
    want *= np.sign((want * e).sum(1))[:, None]
    cs = hitref.curve_state(arr, inst, seg, x)
    assert np.abs(cs["u"] - u).max() < 1e-9 and cs["residual"].max() < 1e-12
    assert np.abs(cs["normal"] - want).max() < 1e-8
    a = c1[:, 3] / np.linalg.norm(c1[:, :3], axis=1)
    assert np.abs(a[seg >= 8]).min() > 0.005 and np.abs(a[seg < 8]).max() < 1e-12  # the second strand tapers, the first does not
    # a cone: four collinear, equally spaced control points with linearly growing radii
    cone = {"curves": np.zeros(1, S.CURVE), "curve_vertex_counts": np.uint32([4]), "curve_points": np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]]),
            "curve_radii": np.float32([0.25, 0.5, 0.75, 1.0]), "instances": np.zeros(1, S.INSTANCE)}
    cone["curves"]["vertex_counts_count"], cone["curves"]["points_count"], cone["curves"]["widths_count"] = 1, 4, 4
    cone["instances"]["transform"][0], cone["instances"]["type"] = np.eye(4)[:3].reshape(12), 2
    cs = hitref.curve_state(cone, 0, np.array([0]), np.array([[1.5, 0.0, 0.625]]))  # c(1/2) = (1.5, 0, 0), r(1/2) = 0.625, r' / |c'| = 1/4
    assert abs(cs["u"][0] - 0.5) < 1e-12 and cs["residual"][0] < 1e-12
    assert np.abs(cs["normal"][0] - unit([-0.25, 0.0, 1.0])).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the normals view
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_flat_normals(name):
    run_cpu(flat_scene(name))


@pytest.mark.parametrize("name", ["nonuniform", "mirror"])
def test_smooth_normals(name):
    """four different vertex normals: barycentrics on the wrong vertices, or the wrong vertex order in one of the two triangles, move the result by many bounds"""
    run_cpu(smooth_scene(name))


@pytest.mark.parametrize("bake", [None, 0])
def test_shared_mesh(bake):
    """one mesh under three transforms, on the baked world-space hierarchy and through a top level"""
    run_cpu(shared_scene(), bake=bake)


@pytest.mark.parametrize("name", ["identity", "nonuniform"])
def test_tilted_vertex_normals(name):
    sc = tilted_scene(name)
    arr = sc.arrays()
    st = hitref.triangle_state(arr, hitref.first_hits(arr, hitref.camera_rays(debug_params(sc), W, H, 0, jitter())))
    ok = np.isfinite(st["kappa"])
    assert np.abs(st["normal"][ok] - st["geom_normal"][ok]).max(axis=1).min() > 0.1  # the view can tell the vertex normal from the face normal
    run_cpu(sc)


TEXELS = [(255, 128, 128), (128, 255, 128), (200, 60, 230)]  # tangent_u, tangent_v, a mix


@pytest.mark.parametrize("texel", TEXELS)
@pytest.mark.parametrize("name", ["nonuniform", "mirror"])
def test_normal_map(name, texel):
    run_cpu(smooth_scene(name, texel), texel)


@pytest.mark.parametrize("name", list(CURVE_TRANSFORMS))
def test_curve_normals(name):
    run_cpu(curve_scene(name), curves=True)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# position and geometric normal, through the rays that leave the first hit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def offset_ray(ork, p, n):
    p, n, out = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(n, np.float32), np.zeros(3, np.float32)
    ork.ork_offset_ray(p.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


POSITION_SCENES = [("flat", n) for n in TRANSFORMS] + [("smooth", "nonuniform"), ("smooth", "mirror"), ("shared", None)]


@pytest.mark.parametrize("kind,name", POSITION_SCENES)
def test_position_and_geometric_normal(ork, kind, name):
    """The origin of the ray that leaves a Lambert surface is offset_ray(position, geom_normal) (tests/test_host_logic.py::test_offset_ray_branches pins that
    function): it equals offset_ray of hitref's float64 position and geometric normal, rounded to float32, within hitref.position_bound per component, and it
    lies on the side of the float64 surface the geometric normal names -- which is the side the camera ray came from.  So does the shadow ray's origin."""
    sc = {"flat": flat_scene, "smooth": smooth_scene}[kind](name) if kind != "shared" else shared_scene()
    arr = sc.arrays()
    v = reference_view(arr, debug_params(sc))
    hit = v["hit"]
    st = hitref.triangle_state(arr, hit)
    o = oracle_for(arr)
    params = debug_params(sc, debug=0, max_depth=2, enable_accumulation=1)
    pick = np.random.RandomState(41).choice(np.nonzero(v["tri"])[0], 200, replace=False)
    assert ((hit["dir"][pick] * st["geom_normal"][pick]).sum(1) < 0).all()  # the camera looks at the side the geometric normal points to
    worst, n_next, n_shadow = 0.0, 0, 0
    for i in pick:
        rows, _ = o.debug_path(params, int(i % W), int(i // W), 0)
        assert rows[0][9] >= 0 and int(rows[0][10]) == hit["inst"][i] and int(rows[0][11]) == hit["prim"][i]
        want = offset_ray(ork, st["position"][i], st["geom_normal"][i])
        bound = hitref.position_bound(st["scale"][i], hit["cos"][i])
        for r in rows[1:3]:
            if r[0] == 1:
                n_shadow += 1
            elif r[0] == 0:
                n_next += 1
            got = r[1:4]
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max() / bound))
            assert (np.abs(got.astype(np.float64) - want) <= bound).all(), (i, got, want, bound)
            assert ((got.astype(np.float64) - st["position"][i]) * st["geom_normal"][i]).sum() > 0, (i, got)
            if r[0] == 0:
                break
    print(f"{kind} {name}: {n_next} bounce and {n_shadow} shadow origins, max |origin - reference| / bound = {worst:.3f}")
    assert n_next >= 180 and n_shadow >= 100
