"""Light shapes on the GPU ("Light shapes"): sampled disk lights and UsdLux shaping cones.  The CPU checker knows neither, so nothing here
is "HIP == oracle": the device functions are held against the float64 statement in tests/lightref.py through skh_light_shape_probe (which calls the `__device__`
functions k_shade calls), the estimator against lightref's quadrature of its own expectation with bounds DERIVED from the scene, and everything that must not
change against the bits of a context that never had a table.

U = 2^-24 is half an ulp, relative: one rounding."""
import math

import numpy as np
import pytest

from strelka_amd import scene as S
from strelka_amd import scenes, tiles
from tests import lightref
from tests.test_gpu_emit import add_triangles, eps, floor_points, one_launch, render

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RHO = 0.5
LI = np.float32([10.0, 6.0, 3.0])
DOWN = S.rotate((1, 0, 0), math.radians(90))  # a disk's local +Z (its normal) turned to world -Y
RECT_DOWN = S.rotate((1, 0, 0), math.radians(-90))  # a rect light emits along local -Z


@pytest.fixture
def ctx():
    from strelka_amd import build, capi

    build.build()
    c = capi.Context(0)
    yield c
    c.close()


def fresh_image(arr, sc, w=32, h=32, n=3, **opts):
    from strelka_amd import capi

    c = capi.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        c.set_scene(arr)
        return render(c, sc, w, h, n)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1: the probe against float64
# ---------------------------------------------------------------------------------------------------------------------------------------------
SKEW = S.rotate((0.3, -0.8, 0.52), 1.1)
CONE = {"coneAngle": math.radians(50.0), "coneSoftness": 0.5, "focus": 2.0}
DISKS = {"small": {"type": 1, "xform": S.translate((0.1, 1.5, -0.2)) @ DOWN, "useXform": True, "radius": 0.05},
         "skew": {"type": 1, "xform": S.translate((0.3, 2.0, 0.1)) @ SKEW, "useXform": True, "radius": 0.45},
         "far": {"type": 1, "xform": S.translate((1e3, 5.0, -1e3)) @ DOWN, "useXform": True, "radius": 5.0}}


def sample_probe(c, light, ux, uy, P):
    rec = np.zeros((len(ux), 6), np.float32)
    rec[:, 1], rec[:, 2], rec[:, 3:6] = ux, uy, P
    rec.view(np.uint32)[:, 0] = light
    o = c.light_shape_probe("sample", rec)
    return {"point": o[:, 0:3], "normal": o[:, 3:6], "L": o[:, 6:9], "dist": o[:, 9], "pdf": o[:, 10], "s": o[:, 11], "area": o[:, 12]}


def pdf_probe(c, light, x, P):
    rec = np.zeros((len(x), 7), np.float32)
    rec[:, 1:4], rec[:, 4:7] = x, P
    rec.view(np.uint32)[:, 0] = light
    o = c.light_shape_probe("pdf", rec)
    return o[:, 0], o[:, 1]


@pytest.mark.parametrize("which", list(DISKS))
def test_probe_against_float64(ctx, which):
    """65 536 draws, ux = (j + 1/2) / N (16 ux is exact: no draw sits on a sector boundary), uy a scrambled copy.  M = |O|_inf + |X|_inf + |Y|_inf bounds every
    coordinate of every vertex.  Bars, one U per rounding:
      point   a vertex: the rounded cosine and sine, two products, two sums: 4 U M; the mapping (three weights of <= 3 U, three products, two sums): 12 U M
              (tests/test_gpu_emit.py::test_probe_values) -> 16 U M per coordinate; off the plane and outside the sector's triangle by at most that x sqrt 3
      normal  normalize: three squares, two sums, the root, the reciprocal, the product: 5 U per component
      area    the cross product's components carry 3 U of |X|_1 |Y|_1 (kappa = 3 |X|_1 |Y|_1 / |X x Y|), then squares, sums, root, constant, product: (kappa + 6) U
      dist    a difference, three squares, two sums, the root: 5 U
      pdf     dist^2 / (cos A) at the RETURNED point: 9 U (dist^2) + (kappa + 6) U (A) + 2 U (product, quotient) + 13 U / cos (the unit direction 5 U, the dot
              product 3 U, the normal 5 U, all relative to the cosine)
      s       c = dot(axis, -L) carries 8 U absolute (L 5 U, the dot 3 U); t moves by that / (cos_inner - cos_outer), the smoothstep's slope is <= 1.5, pow's
              <= focus; the evaluation itself 23.6 U relative (tests/test_lightshape_cpu.py): |s - s64| <= 24 U s + 8 U (1.5 / (ci - co) + focus)."""
    sc = S.Scene()
    lid = sc.createLight({**DISKS[which], "sample": True, **CONE, "color": (1, 1, 1)})
    arr = sc.arrays()
    ctx.set_scene(arr, build=False)
    assert ctx.light_shape_info() == {"sampled_discs": 1, "cones": 1}
    l, sh = arr["lights"][lid], arr["light_shapes"][lid]
    O, X, Y = (l["points"][k][:3].astype(np.float64) for k in (1, 2, 3))
    n64 = l["normal"][:3].astype(np.float64)
    r = float(np.linalg.norm(n64))
    n64 /= r
    assert abs(r / DISKS[which]["radius"] - 1) < 1e-6  # (the reference stores the normal scaled by the radius)
    A = lightref.disc_area(X, Y)
    M = np.abs(O).max() + np.abs(X).max() + np.abs(Y).max()
    N = 65536
    rs = np.random.RandomState(41)
    ux = ((np.arange(N) + 0.5) / N).astype(np.float32)
    uy = ((rs.permutation(N) + 0.5) / N).astype(np.float32)
    assert (ux.astype(np.float64) * N - 0.5 == np.arange(N)).all()
    # shaded points: in front of the disk, 1 ... 8 radii away, a quarter of them behind it
    side = np.where(np.arange(N) % 4 == 3, -1.0, 1.0)
    P = (O + rs.uniform(-4, 4, (N, 1)) * X + rs.uniform(-4, 4, (N, 1)) * Y + (side * rs.uniform(1, 8, N))[:, None] * r * n64).astype(np.float32)
    s = sample_probe(ctx, lid, ux, uy, P)
    k, up = lightref.sector(ux.astype(np.float64))
    assert np.array_equal(k, np.floor(16 * ux.astype(np.float64))) and np.array_equal(np.bincount(k, minlength=16), np.full(16, 4096))
    pt = s["point"].astype(np.float64)
    want = lightref.disc_point(O, X, Y, ux.astype(np.float64), uy.astype(np.float64))
    e_pt = np.abs(pt - want).max() / M
    # inside the sector's own triangle (O, v_k, v_k+1) -- hence inside the 16-gon --: barycentrics >= -bar, on the plane
    v = lightref.disc_vertices(O, X, Y)
    e1, e2, d = v[k] - O, v[k + 1] - O, pt - O
    den = np.cross(e1, e2) @ n64
    b1, b2 = (np.cross(d, e2) @ n64) / den, (np.cross(e1, d) @ n64) / den
    slack = 16 * math.sqrt(3) * U * M / np.linalg.norm(e1, axis=1).min() * 3  # a distance of 16 sqrt 3 U M as a barycentric coordinate: the sector's height is sin(22.5 deg) = 0.38 of its side
    inside = min(b1.min(), b2.min(), (1 - b1 - b2).min())
    e_plane = np.abs(d @ n64).max() / M
    e_n = np.abs(s["normal"] - n64).max()
    e_area = np.abs(s["area"].astype(np.float64) / A - 1).max()
    dvec = pt - P.astype(np.float64)
    dist = np.linalg.norm(dvec, axis=1)
    e_dist = np.abs(s["dist"] / dist - 1).max()
    cos_l = -(dvec @ n64) / dist
    front, behind = cos_l > 1e-3, cos_l < -1e-3
    kappa = 3 * np.abs(X).sum() * np.abs(Y).sum() / np.linalg.norm(np.cross(X, Y))
    want_pdf = lightref.area_pdf(n64, A, pt, P.astype(np.float64))
    bar_pdf = (kappa + 17) * U + 13 * U / np.where(front, cos_l, 1.0)
    rel_pdf = np.abs(s["pdf"].astype(np.float64) - want_pdf) / np.where(front, want_pdf, 1.0)
    co, ci, focus, axis = lightref.shape_of(sh)
    want_s = lightref.s_cone(-(dvec / dist[:, None]) @ axis, co, ci, focus)
    bar_s = 24 * U * want_s + 8 * U * (1.5 / (ci - co) + focus)
    e_s = np.abs(s["s"] - want_s) / bar_s
    print(f"{which}: point {e_pt / U:.2f} U M (bar 16), plane {e_plane / U:.2f} U M (bar {16 * math.sqrt(3):.1f}), min barycentric {inside:.2e} (bar {-slack:.2e}), "
          f"normal {e_n / U:.2f} U (bar 5), area {e_area / U:.2f} U (bar {kappa + 6:.1f}), dist {e_dist / U:.2f} U (bar 5), pdf / bar {(rel_pdf[front] / bar_pdf[front]).max():.3f}, "
          f"s / bar {e_s.max():.3f}; lit {float((want_s > 0).mean()):.2f}, from behind {int(behind.sum())}")
    assert e_pt <= 16 * U and e_plane <= 16 * math.sqrt(3) * U and inside >= -slack
    assert e_n <= 5 * U and e_area <= (kappa + 6) * U and e_dist <= 5 * U
    assert (rel_pdf[front] <= bar_pdf[front]).all() and front.sum() > N // 2
    assert (s["pdf"][behind] == 0).all() and behind.sum() > N // 8  # a point seen from behind gives pdf 0
    assert (e_s <= 1).all() and 0.05 < (want_s > 0).mean() < 0.95
    # the PDF probe at the sampled point: the same functions on the same values, the same bits
    pp, ps = pdf_probe(ctx, lid, s["point"], P)
    assert np.array_equal(pp.view(np.uint32), s["pdf"].view(np.uint32)) and np.array_equal(ps.view(np.uint32), s["s"].view(np.uint32))


def test_probe_of_the_other_light_types(ctx):
    """types 0, 2 and 3 answer with the existing samplers' bits (SKH_UNIT_LIGHT_SAMPLE), s applied when a cone is set; a disk without the flag with zeros"""
    sc = scenes.spot_room()
    sc.createLight({"type": 3, "xform": S.rotate((1, 0, 0), math.radians(-60)), "useXform": True, "halfAngle": math.radians(3.0), "radius": 0.0})
    sc.createLight({"type": 1, "xform": S.translate((0, 2.9, 0)) @ DOWN, "useXform": True, "radius": 0.3})  # not sampled
    arr = sc.arrays()
    ctx.set_scene(arr, build=False)
    rs = np.random.RandomState(2)
    n = 4096
    ux, uy = rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32)
    P = (rs.rand(n, 3) * [3, 1.5, 3] - [1.5, 0, 1.5]).astype(np.float32)
    for lid, kind in ((0, 2), (2, 0), (3, 3)):
        s = sample_probe(ctx, lid, ux, uy, P)
        rec = np.concatenate([P, ux[:, None], uy[:, None]], 1).astype(np.float32)
        o = ctx.unit_probe("light_sample", rec, param=kind, consts=arr["lights"][lid:lid + 1]).view(np.float32)
        for name, col in (("point", slice(0, 3)), ("normal", slice(4, 7)), ("L", slice(8, 11))):
            assert np.array_equal(s[name].view(np.uint32), o[:, col].view(np.uint32)), (lid, name)
        assert np.array_equal(s["pdf"].view(np.uint32), o[:, 3].view(np.uint32)) and np.array_equal(s["dist"].view(np.uint32), o[:, 11].view(np.uint32))
        shape = lightref.shape_of(arr["light_shapes"][lid])
        want = lightref.shape_s(shape, -s["L"].astype(np.float64))
        if shape is None:
            assert (s["s"] == 1).all()
        else:
            co, ci, focus, _ = shape  # (the bar of test_probe_against_float64; L is the device's own here: 3 U for the dot product alone would do)
            assert (np.abs(s["s"] - want) <= 24 * U * want + 8 * U * (1.5 / (ci - co) + focus)).all()
            assert 0.02 < (want > 0).mean() < 0.98
    z = sample_probe(ctx, 4, ux, uy, P)
    assert all((z[k] == 0).all() for k in ("point", "normal", "L", "dist", "pdf", "area"))
    assert (sample_probe(ctx, 99, ux[:4], uy[:4], P[:4])["pdf"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2, 3: the estimator against its integral
# ---------------------------------------------------------------------------------------------------------------------------------------------
VIEWS = {"under": ((3.0, 1.0, 0.4), (0.0, 0.0, 0.0)), "off_axis": ((5.0, 1.0, 1.4), (2.0, 0.0, 1.0)), "edge": ((3.6, 1.0, 0.4), (0.6, 0.0, 0.0)),
         "outside": ((6.0, 1.0, 1.4), (3.0, 0.0, 1.0))}
DISK = {"type": 1, "xform": S.translate((0.0, 1.5, 0.0)) @ DOWN, "useXform": True, "radius": 0.5, "color": tuple(float(v) for v in LI), "intensity": 1.0}
SPHERE = {"type": 2, "xform": S.translate((0.0, 1.5, 0.0)), "useXform": True, "radius": 0.1, "color": tuple(float(v) for v in LI), "intensity": 1.0}
RECT = {"type": 0, "xform": S.translate((0.0, 1.5, 0.0)) @ RECT_DOWN, "useXform": True, "width": 1.0, "height": 0.6, "color": tuple(float(v) for v in LI),
        "intensity": 1.0}
BELOW = {"type": 0, "xform": S.translate((0.0, -1.5, 0.0)) @ RECT_DOWN, "useXform": True, "width": 1.0, "height": 0.6, "color": (10.0, 10.0, 10.0), "intensity": 1.0}


def floor_scene(lights, view):
    """tests/test_gpu_emit.py's floor: rho = 0.5, 40 x 40, seen through 8 x 8 pixels of a 1.5 degree camera; nothing the floor reflects comes back to it"""
    sc = S.Scene()
    grey = sc.addMaterial(S.MAT_DIFFUSE, (RHO, RHO, RHO))
    add_triangles(sc, np.float32([[(-20, 0, 20), (20, 0, 20), (20, 0, -20)], [(-20, 0, 20), (20, 0, -20), (-20, 0, -20)]]), grey)
    for d in lights:
        sc.createLight(d)
    cam = S.Camera(fov=1.5)
    cam.lookAt(*VIEWS[view])
    sc.addCamera(cam)
    return sc


def light_mu(arr, lid, p, num_pick, sampled=True, m=1):
    """mu(p) / (rho Li) of light `lid` of the scene for floor points p (..., 3): lightref's quadrature of the estimator's expectation"""
    l = arr["lights"][lid]
    shapes = arr.get("light_shapes")
    shape = None if shapes is None else lightref.shape_of(shapes[lid])
    typ = int(l["type"])
    up = (0.0, 1.0, 0.0)
    if typ == 1:
        O, X, Y = (l["points"][k][:3].astype(np.float64) for k in (1, 2, 3))
        n = l["normal"][:3].astype(np.float64)
        r = np.linalg.norm(n)
        pts, dA = lightref.disc_cells(O, X, Y, 24 * m)
        f = lambda q: lightref.area_light_mu(pts, dA, n / r, lightref.disc_area(X, Y), q, up, num_pick, shape, sampled, hit_scale=r)
    elif typ == 0:
        pp = l["points"][:, :3].astype(np.float64)
        n = -np.cross(pp[1] - pp[0], pp[3] - pp[0])
        area = np.linalg.norm(n)
        pts, dA = lightref.rect_cells(l["points"], 96 * m)
        f = lambda q: lightref.area_light_mu(pts, dA, n / area, area, q, up, num_pick, shape)
    else:
        tris = lightref.proxy_triangles(arr, lid)
        f = lambda q: lightref.sphere_light_mu(l["points"][1][:3], float(l["points"][0][0]), tris, q, up, num_pick, shape, m_dir=64 * m)
    p = np.asarray(p, np.float64)
    return np.array([f(q) for q in p.reshape(-1, 3)]).reshape(p.shape[:-1])


def pick_n(mu, vmax, extra):
    """the smallest power of two that puts 6 sqrt(V / (P N)) + eps(N) mu + extra below 10 % of mu, V <= mu (vmax - mu) (Bhatia-Davis: a sample lies in [0, vmax])"""
    for k in range(8, 21):
        N = 1 << k
        bound = 6 * np.sqrt(mu * (vmax - mu) / (64 * N)) + eps(N) * mu + extra
        if (bound <= 0.1 * mu).all():
            return N, bound
    return None, bound


def expectation(arr, sc, lid, num_pick, sampled=True):
    """per pixel mu (8, 8, 3), its mean, and what the bound adds to the sampling term: the spread of mu over a pixel (its corners against its centre) and the
    quadrature's own error, taken as twice the change from halving its cells (the midpoint rule converges at least linearly, also across a hard cone edge)"""
    fp = floor_points(sc, 8, 8)
    g = light_mu(arr, lid, fp, num_pick, sampled)  # (8, 8, 5)
    fine = light_mu(arr, lid, fp[:, :, 0], num_pick, sampled, m=2)
    rl = RHO * LI.astype(np.float64)
    mu_px = g[:, :, 0, None] * rl
    spread = np.abs(g[:, :, 1:] - g[:, :, :1]).max(axis=2).mean() * rl
    quad = 2 * np.abs(fine - g[:, :, 0]).mean() * rl
    return mu_px, mu_px.mean(axis=(0, 1)), spread + quad, fp


@pytest.mark.parametrize("view,below", [("under", False), ("off_axis", False), ("under", True), ("off_axis", True)])
def test_sampled_disk_against_its_integral(ctx, view, below):
    """A black-based disk light of radius 0.5 at height 1.5 shines down on the floor; one launch of N samples; the mean over the P = 64 pixels, per channel:
    |mean - mu| <= 6 sqrt(V / (P N)) + eps(N) mu + spread (+ the quadrature's error), mu from lightref (its docstring has the integrand: the rect branch of
    k_shade read term by term).  Flag on: each technique's weighted sample is <= rho Li (light sampling: lrad bsdf / (p_L + p_B) <= Li cos_s rho; BSDF sampling:
    rho Li cos_l w_B), their sum in [0, 2 rho Li] -> V <= mu (2 rho Li - mu).  Flag off: the light is what it always was -- hits only, Li r cos_l with the
    reference's radius-scaled normal, weight 1 -- a sample lies in [0, rho Li r] -> V <= mu (rho Li r - mu); held against ITS integral.  N: the smallest power of
    two that puts both bounds below 10 % of mu.  A rect light UNDER the floor lights nothing and takes half the picks: a wrong 1 / numPick shows.  The reason the
    feature exists: the relative per-pixel MSE (MSE / mu^2) is smaller with the flag than without."""
    lights = [DISK] + ([BELOW] if below else [])
    num_pick = len(lights)
    rl = RHO * LI.astype(np.float64)
    runs = {}
    for on in (True, False):
        sc = floor_scene([{**DISK, "sample": True}] + lights[1:] if on else lights, view)
        arr = sc.arrays()
        mu_px, mu, extra, _ = expectation(arr, sc, 0, num_pick, sampled=on)
        runs[on] = (sc, arr, mu_px, mu, extra, pick_n(mu, (2.0 if on else 0.5) * rl, extra))
    assert all(r[5][0] is not None for r in runs.values()), [r[5] for r in runs.values()]
    N = max(r[5][0] for r in runs.values())
    rel_mse = {}
    for on, (sc, arr, mu_px, mu, extra, _) in runs.items():
        bound = 6 * np.sqrt(mu * ((2.0 if on else 0.5) * rl - mu) / (64 * N)) + eps(N) * mu + extra
        ctx.set_scene(arr)
        assert ctx.light_shape_info()["sampled_discs"] == int(on)
        ctx.reset_stats()
        img = one_launch(ctx, sc, N, 4)
        mean = img.mean(axis=(0, 1))
        rel_mse[on] = float((((img - mu_px) / mu_px) ** 2).mean())
        shadow = ctx.stats()["rays_shadow"]
        print(f"{view} below {below} flag {on}: N {N}, mean {mean}, mu {mu}, |diff| / bound {np.abs(mean - mu) / bound}, bound / mu {bound / mu}, "
              f"relative per-pixel MSE {rel_mse[on]:.4e}, shadow rays {shadow}")
        assert (bound <= 0.1 * mu).all()
        assert (np.abs(mean - mu) <= bound).all(), (on, mean, mu, bound)
        assert (shadow > 0) == on  # (an unflagged disk returns the zero sample; the light under the floor is below the horizon)
    assert rel_mse[True] < rel_mse[False], rel_mse


CONE_CASES = {"sphere": ({**SPHERE, "coneAngle": math.radians(30.0), "axis": (0.0, -1.0, 0.0)}, "under", 0.1),
              "rect": ({**RECT, "coneAngle": math.radians(40.0), "coneSoftness": 0.5, "focus": 2.0}, "under", math.hypot(0.5, 0.3)),
              "disk": ({**DISK, "sample": True, "coneAngle": math.radians(25.0)}, "edge", 0.5)}


@pytest.mark.parametrize("which", list(CONE_CASES))
def test_cone_against_its_integral(ctx, which):
    """the same floor and the same bound, mu from the quadrature with s in it: a sphere light of radius 0.1 under a hard 30 degree cone (the floor under it is
    inside: s = 1 there, the cone must not darken it), a rect light with angle 40, softness 0.5 and focus 2 (s falls from 1 to 0.87 over the light as seen from
    the floor), the sampled disk under a hard 25 degree cone seen from 0.6 off its axis (part of the disk is dark for every floor point: the edge runs through the
    light).  s <= 1, so every sample bound of the test above holds.  The sphere light's estimator is the reference's (uniform over the whole sphere, called
    1 / 4 pi per solid angle; lightref.sphere_light_mu integrates exactly that, the hit term over the proxy's own faces)."""
    desc, view, _ = CONE_CASES[which]
    sc = floor_scene([desc], view)
    arr = sc.arrays()
    mu_px, mu, extra, _ = expectation(arr, sc, 0, 1)
    rl = RHO * LI.astype(np.float64)
    N, bound = pick_n(mu, 2.0 * rl, extra)
    assert N is not None, (mu, extra)
    ctx.set_scene(arr)
    assert ctx.light_shape_info()["cones"] == 1
    ctx.reset_stats()
    img = one_launch(ctx, sc, N, 4)
    mean = img.mean(axis=(0, 1))
    mu0 = mu
    if which != "sphere":  # (under the sphere light s = 1 on this floor)
        plain = {k: v for k, v in desc.items() if k not in ("coneAngle", "coneSoftness", "focus", "axis")}
        sc0 = floor_scene([plain], view)
        mu0 = expectation(sc0.arrays(), sc0, 0, 1)[1]
    print(f"{which} {view}: N {N}, mean {mean}, mu {mu} (without the cone {mu0}), |diff| / bound {np.abs(mean - mu) / bound}, bound / mu {bound / mu}, "
          f"shadow rays {ctx.stats()['rays_shadow']}")
    assert (bound <= 0.1 * mu).all()
    assert (np.abs(mean - mu) <= bound).all(), (mean, mu, bound)
    if which != "sphere":
        assert (mu < 0.98 * mu0).all()  # the cone matters in this view: the test would notice a missing s


@pytest.mark.parametrize("which", list(CONE_CASES))
def test_outside_the_cone_is_exactly_dark(ctx, which):
    """a view whose 64 floor points all lie outside the cone: lateral offset >= h tan(angle) + the light's extent + 0.2.  lightref confirms s = 0 from every
    light point first; then the image is exactly 0 and no shadow ray was queued."""
    desc, _, extent = CONE_CASES[which]
    sc = floor_scene([desc], "outside")
    arr = sc.arrays()
    fp = floor_points(sc, 8, 8).reshape(-1, 3)
    lateral = np.hypot(fp[:, 0], fp[:, 2]).min()
    assert lateral >= 1.5 * math.tan(desc["coneAngle"]) + extent + 0.2
    shape = lightref.shape_of(arr["light_shapes"][0])
    tris = lightref.proxy_triangles(arr, 0)
    x = np.concatenate([tris.reshape(-1, 3), lightref.triangle_cells(tris, 3)[0]])
    if which == "sphere":  # the analytic sphere's points too: the sampler draws from it
        u = np.random.RandomState(1).normal(size=(4096, 3))
        x = np.concatenate([x, np.array([0.0, 1.5, 0.0]) + 0.1 * u / np.linalg.norm(u, axis=1)[:, None]])
    w = fp[None, :, :] - x[:, None, :]
    w /= np.linalg.norm(w, axis=2)[:, :, None]
    assert (lightref.shape_s(shape, w) == 0).all()
    ctx.set_scene(arr)
    ctx.reset_stats()
    img = one_launch(ctx, sc, 1024, 4)
    st = ctx.stats()
    assert (img == 0).all() and st["rays_shadow"] == 0 and st["rays_radiance"] > 64 * 1024
    # (the same view without the cone is lit: the darkness is the cone's)
    plain = {k: v for k, v in desc.items() if k not in ("coneAngle", "coneSoftness", "focus", "axis")}
    sc0 = floor_scene([plain], "outside")
    ctx.set_scene(sc0.arrays())
    assert one_launch(ctx, sc0, 256, 4).mean() > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4: nothing changes without a shape
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["light_zoo", "hair"])
def test_nothing_changes_without_a_shape(ctx, which):
    sc = scenes.light_zoo() if which == "light_zoo" else scenes.hair_standin(seed=5, n_strands=1500, n_cp=8)
    arr = sc.arrays()
    assert "light_shapes" not in arr
    ctx.set_scene(arr)
    want = render(ctx, sc, 32, 32, 3)  # the context before any table was set
    assert want.max() > 0 and ctx.light_shape_info() == {"sampled_discs": 0, "cones": 0}
    nl = len(arr["lights"])
    ctx.set_light_shapes(None)
    assert np.array_equal(render(ctx, sc, 32, 32, 3), want)
    ctx.set_light_shapes(np.zeros(nl, S.LIGHT_SHAPE))
    assert ctx.light_shape_info() == {"sampled_discs": 0, "cones": 0}
    assert np.array_equal(render(ctx, sc, 32, 32, 3), want)
    t = np.zeros(nl, S.LIGHT_SHAPE)
    rect = int(np.flatnonzero(arr["lights"]["type"] == 0)[0])
    t[rect]["flags"] = S.LIGHT_SHAPE_SAMPLE_DISC  # does not apply to a rect light
    if which == "light_zoo":
        t[3]["flags"] = S.LIGHT_SHAPE_SAMPLE_DISC | S.LIGHT_SHAPE_CONE  # nor does either to a distant light
        t[3]["axis"] = (0, -1, 0)
    ctx.set_light_shapes(t)
    assert ctx.light_shape_info() == {"sampled_discs": 0, "cones": 0}
    assert np.array_equal(render(ctx, sc, 32, 32, 3), want)
    # a shape in use changes the image ...
    t[rect]["flags"], t[rect]["cos_outer"], t[rect]["cos_inner"] = S.LIGHT_SHAPE_CONE, math.cos(math.radians(12)), math.cos(math.radians(8))
    L = arr["lights"][rect]["points"][:, :3].astype(np.float64)
    a = -np.cross(L[1] - L[0], L[3] - L[0])
    t[rect]["axis"] = a / np.linalg.norm(a)
    ctx.set_light_shapes(t)
    assert ctx.light_shape_info()["cones"] == 1
    lit = render(ctx, sc, 32, 32, 3)
    assert not np.array_equal(lit, want) and np.isfinite(lit).all()
    # ... and removing the table brings the bits back
    ctx.set_light_shapes(None)
    assert ctx.light_shape_info() == {"sampled_discs": 0, "cones": 0}
    assert np.array_equal(render(ctx, sc, 32, 32, 3), want)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5: options and scheduling
# ---------------------------------------------------------------------------------------------------------------------------------------------
def hair_under_a_spot():
    """a tiny hair scene under a coned sphere light: the HAIR x LSHAPE build"""
    sc = scenes.hair_standin(seed=5, n_strands=400, n_cp=8)
    sc.createLight({"type": 2, "xform": S.translate((0.5, 2.5, 1.5)), "useXform": True, "radius": 0.2, "color": (1.0, 0.9, 0.8), "intensity": 60.0,
                    "coneAngle": math.radians(35.0), "coneSoftness": 0.4, "axis": (-0.2, -0.85, -0.5)})
    return sc


@pytest.mark.parametrize("which,bake", [("spot_room", 4), ("spot_room", 0), ("hair", 4)])
def test_options_leave_a_shaped_image_bit_identical(ctx, which, bake):
    """the options tests/test_gpu_emit.py::test_options_leave_an_emitter_lit_image_bit_identical runs: speculation through per-sub-frame calls, sub-frame
    batches, a two-tile ownership split; once per hierarchy kind (bake_world is part of the intersection's definition: compared within a setting)"""
    sc = scenes.spot_room() if which == "spot_room" else hair_under_a_spot()
    arr = sc.arrays()
    ctx.set_option("bake_world", bake)
    ctx.set_scene(arr)
    info = ctx.light_shape_info()
    assert info == ({"sampled_discs": 1, "cones": 2} if which == "spot_room" else {"sampled_discs": 0, "cones": 1})
    w, h, spp = 32, 32, 12

    def frame(batch=False):
        ctx.resize(w, h)
        if not batch:
            return render(ctx, sc, w, h, spp)
        ctx.render_subframes(S.frame_params(sc.getCamera(), w, h, subframe_index=0, spp_total=spp, max_depth=4), spp)
        return ctx.read_accum()[..., :3].copy()

    ctx.set_option("speculate", 0)
    base = frame()
    assert base.max() > 0 and np.isfinite(base).all()
    ctx.reset_stats()
    ctx.set_option("speculate", 8)
    assert np.array_equal(frame(), base)
    ctx.set_option("subframe_batch", 1)
    assert np.array_equal(frame(batch=True), base)
    ctx.set_option("subframe_batch", 0)
    assert np.array_equal(frame(batch=True), base)
    full = np.zeros((h, w, 3), np.float32)
    T = 16
    for rank in range(2):
        txy = tiles.assign_tiles(w, h, T, 2, rank)
        ctx.set_tiles(T, txy)
        part = frame()
        for (x0, y0) in np.asarray(txy).reshape(-1, 2):
            full[y0:y0 + T, x0:x0 + T] = part[y0:y0 + T, x0:x0 + T]
    ctx.set_tiles(32, None)
    assert np.array_equal(full, base)
    # the shapes matter in this picture, and a fresh context given the same scene draws the same bits
    assert np.array_equal(fresh_image(arr, sc, w, h, spp, bake_world=bake), base)
    plain = {k: v for k, v in arr.items() if k != "light_shapes"}
    assert not np.array_equal(fresh_image(plain, sc, w, h, spp, bake_world=bake), base)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6: the table follows the scene
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_follows_the_light_list(ctx):
    sc = scenes.spot_room()
    arr = sc.arrays()  # lights: sphere + cone, disk + sample, rect + cone
    ctx.set_scene(arr)
    assert ctx.light_shape_info() == {"sampled_discs": 1, "cones": 2}
    base = render(ctx, sc, 32, 32, 3)
    # a shorter list: the surplus entries are unused (the proxies of the lights that left answer as light 0, as they always did)
    ctx.set_lights(arr["lights"][:1])
    assert ctx.light_shape_info() == {"sampled_discs": 0, "cones": 1}
    short = render(ctx, sc, 32, 32, 3)
    assert np.isfinite(short).all() and not np.array_equal(short, base)
    # other types under the same entries: the cone of entry 0 now sits on the disk, SAMPLE_DISC of entry 1 on the sphere light (does not apply)
    ctx.set_lights(arr["lights"][[1, 0, 2]])
    assert ctx.light_shape_info() == {"sampled_discs": 0, "cones": 2}
    assert np.isfinite(render(ctx, sc, 32, 32, 3)).all()
    # the list of before: the table of before, the bits of before
    ctx.set_lights(arr["lights"])
    assert ctx.light_shape_info() == {"sampled_discs": 1, "cones": 2}
    assert np.array_equal(render(ctx, sc, 32, 32, 3), base)
    # a setter between two sub-frames of a speculated frame shows in the very next one
    P = lambda i: S.frame_params(sc.getCamera(), 32, 32, subframe_index=i, spp_total=8, max_depth=4)
    images = []
    for spec in (8, 0):
        ctx.set_option("speculate", spec)
        ctx.set_light_shapes(arr["light_shapes"])
        ctx.resize(32, 32)
        ctx.reset_stats()
        for i in range(5):
            ctx.render_subframe(P(i))
        ctx.set_light_shapes(arr["light_shapes"][:1])
        ctx.render_subframe(P(5))
        images.append(ctx.read_accum()[..., :3].copy())
        if spec:
            assert ctx.stats()["speculated_discarded"] > 0
    assert np.array_equal(images[0], images[1])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7: refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_tables_are_refused_and_the_previous_one_stays(ctx):
    from strelka_amd import capi

    sc = scenes.spot_room()
    arr = sc.arrays()
    ctx.set_scene(arr)
    good = arr["light_shapes"]
    info = ctx.light_shape_info()
    a = render(ctx, sc, 32, 32, 2)

    def bad(i, **kw):
        t = good.copy()
        for k, v in kw.items():
            t[i][k] = v
        return t

    cases = [bad(0, flags=4), bad(1, flags=7), bad(0, cos_outer=1.5), bad(0, cos_outer=-1.5, cos_inner=0.0), bad(0, cos_inner=np.nan), bad(0, cos_outer=np.inf),
             bad(0, cos_inner=1.25), bad(2, cos_outer=0.5, cos_inner=0.25), bad(0, focus=-1.0), bad(0, focus=np.inf), bad(0, focus=np.nan),
             bad(0, axis=(0.0, -2.0, 0.0)), bad(0, axis=(0.0, 0.0, 0.0)), bad(0, axis=(0.0, -0.998, 0.0)), bad(2, axis=(np.nan, 0.0, 1.0)),
             bad(2, axis=(np.inf, 0.0, 0.0)), bad(1, reserved=1), np.zeros(len(good) + 1, S.LIGHT_SHAPE)]
    for t in cases:
        with pytest.raises(capi.SkhError) as ei:
            ctx.set_light_shapes(t)
        assert "(3)" in str(ei.value)  # SKH_INVALID_ARGUMENT
        assert ctx.light_shape_info() == info
    assert ctx.lib.skh_light_shape_probe(ctx.h, 2, None, 0, None) == 3  # an unknown kind
    assert np.array_equal(render(ctx, sc, 32, 32, 2), a)  # the previous table is in place: the bits of before
    # an axis off unit length by less than 1e-3 and an axis of any kind without CONE are accepted
    ok = bad(0, axis=(0.0, -1.0005, 0.0))
    ok[1]["axis"] = (5.0, 0.0, 0.0)
    ctx.set_light_shapes(ok)
    ctx.set_light_shapes(good)
    assert ctx.light_shape_info() == info
    assert np.array_equal(render(ctx, sc, 32, 32, 2), a) and np.isfinite(a).all()
