"""The device's curve path at HAIR scale against float64 directly ("Curve intersection against float64"): `skh_trace` hit records held to
tests/curveref.py with the bars of tests/test_curve_hairscale_cpu.py -- written-out counts of roundings relative to the radius and the distance --, no checker in
between.  The checker is compared bit for bit on the same rays AFTER the float64 judgement, so a failure says which side moved.

What only the device has, and where it is visited: the bounding-cylinder cull and the parameter sub-range boxes (curve_split 1, 2, 5, 8), the merged / world-curve trees
and the two-level kernel (one prim; two prims under a shared transform; three under their own), the per-instance ray transform at a curve root (rotation + non-uniform
scale; a translation by 1e3), the cooperative Newton block with many lanes parked at once (40 hairs within 3 r of each other met by 64 rays in a line), per-ray tmin / tmax
next to the entry, rays along the axes with -0.0 components, and a mesh 2 r behind the hair.

Scenes are 64 strands x 8 control points, radii 4e-4 -> 1e-4 (the hair stand-in's), <= 4 000 rays a case; the float64 reference of a scene is computed once.

INJECTED ERRORS (each a one-line change to a scratch copy of the device's or the checker's text, built beside the shipped library and run through these files; none is
committed).  "caught by" names the assertion that failed first -- the float64 judgement stands in front of the comparison with the checker in every test:
  1. convergence threshold 5e-5 -> 5e-4       device: all 19 tests here fail on `|u - u_foot| <= bar_u` (7.4 ... 8.5 bar_u); checker: the three checker tests of
                                               tests/test_curve_hairscale_cpu.py fail on the same bar (7.6 bar_u).
  2. on-tube factor 1.001 -> 1.05              NOT caught by either file, and it cannot be by rays the decided set admits: the factor only gates roots of a degenerate
                                               cone quadratic (a ray along the tangent); a ray at >= 20 degrees that passes the tube has no real root to accept.  Rays
                                               along the tangent of THICK tubes passing at 1.00 ... 1.06 r do show it on the checker (reported points up to 0.0247 r off
                                               the surface against 0.0030 r as shipped), but that is the tangent case, which has its own test
                                               (tests/test_oracle_intersect.py; its bar, 1e-3 + 0.02 r, does not see 1.05 either).  Left open: DESIGN.md.
  3. cylinder cull's radius x 0.98             device: test_grazing_hits_on_straight_strands_survive_the_cull fails on "decision agrees" (173 decided hits lost); the
                                               other 18 pass -- on a bent hair, and with curve_split > 1 (2 r_max of pad), the cylinder is looser than 2 %.
  4. sub-range box without its radius pad      device: 12 tests fail on "decision agrees" (2 ... 15 decided hits lost a case): curve_split 4 (the default), 5 and 8 under
                                               every transform, the axis rays, the scalp scene; curve_split 1 and 2, the bundle and the straight strands pass (the hull of
                                               a long sub-range's Bezier points is loose enough).
  5. u reported as 1 - u                       device: all 19 fail on `|u - u_foot| <= bar_u` (1e4 bar_u); checker: the three checker tests likewise.
"""
import numpy as np
import pytest

from strelka_amd import scene as S
from tests import curveref as R
from tests.hitref import bspline

pytestmark = pytest.mark.gpu

R_ROOT, R_TIP = 4e-4, 1e-4
MISS = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def strands(seed, n=64, n_cp=8, extent=0.12, step=(0.03, 0.09)):
    """n strands of n_cp control points in a box of +-extent, steps of 0.03 ... 0.09 bending a few degrees each, radius 4e-4 at the root -> 1e-4 at the tip:
    -> points (n, n_cp, 3), radii (n, n_cp), float32"""
    rs = np.random.RandomState(seed)
    pts = np.zeros((n, n_cp, 3))
    for s in range(n):
        p = rs.uniform(-extent, extent, 3)
        d = rs.normal(size=3)
        d /= np.linalg.norm(d)
        for k in range(n_cp):
            pts[s, k] = p
            d = d + 0.15 * rs.normal(size=3)
            d /= np.linalg.norm(d)
            p = p + d * rs.uniform(*step)
    rad = np.broadcast_to(np.linspace(R_ROOT, R_TIP, n_cp)[None, :], (n, n_cp))
    return pts.astype(np.float32), rad.astype(np.float32)


def bundle(seed, n=40, n_cp=8, r=2e-4):
    """n hairs of radius r whose axes lie within 3 r of each other: one gently bent strand, copied with offsets inside a disc of radius 1.5 r across it"""
    rs = np.random.RandomState(seed)
    base, _ = strands(seed, 1, n_cp, 0.02, (0.05, 0.06))
    axis = base[0, -1] - base[0, 0]
    axis = axis / np.linalg.norm(axis)
    a = np.cross(axis, [0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    b = np.cross(axis, a)
    rr, ph = 1.5 * r * np.sqrt(rs.uniform(0, 1, n)), rs.uniform(0, 2 * np.pi, n)
    off = rr[:, None] * (np.cos(ph)[:, None] * a + np.sin(ph)[:, None] * b)
    pts = base.astype(np.float64) + off[:, None, :]
    return pts.astype(np.float32), np.full((n, n_cp), r, np.float32)


XF = {
    "identity": [np.eye(4)],
    "rotated_scaled": [S.translate((0.1, -0.2, 0.05)) @ S.rotate((0.3, 1.0, 0.2), 0.7) @ S.scale((1.3, 0.8, 1.1))],
    "far": [S.translate((1000.0, -1000.0, 1000.0))],
    "two_shared": [S.translate((0.1, 0.0, -0.05)) @ S.rotate((0, 1, 0), 0.4)] * 2,
    "three_own": [S.translate((0.4, 0.0, 0.0)) @ S.rotate((0, 0, 1), 0.3), S.translate((-0.4, 0.1, 0.0)) @ S.rotate((1, 0, 0), -0.5) @ S.scale((0.9, 1.2, 1.0)), S.translate((0.0, -0.4, 0.2))],
}


def make_scene(pts, rad, matrices, mesh_z=None):
    """the strands dealt round-robin to len(matrices) curve sets, one instance each under its matrix (the points are object-space); mesh_z: a quad z = mesh_z spanning
    +-1 in x and y (a scalp stand-in), identity"""
    sc = S.Scene()
    sc.addMaterial()
    mat = sc.addHairMaterial()
    if mesh_z is not None:
        vb, ib = S.deindex([(-1, -1, mesh_z), (1, -1, mesh_z), (1, 1, mesh_z), (-1, 1, mesh_z)], [(0, 1, 2), (0, 2, 3)])
        sc.createInstance(S.INSTANCE_MESH, sc.createMesh(vb, ib), 0, np.eye(4))
    for k, M in enumerate(matrices):
        p, r = pts[k::len(matrices)], rad[k::len(matrices)]
        cid = sc.createCurve(np.full(len(p), p.shape[1], np.uint32), p.reshape(-1, 3), r.reshape(-1))
        sc.createInstance(S.INSTANCE_CURVE, cid, mat, M)
    return sc.arrays()


def aim(arr, n, seed, distances=(0.3, 3.0), dlens=(1.0, 37.0, 1.0 / 37.0), axes=False):
    """n rays at random segments of the scene's curve instances: through C(u0) + rho r w in OBJECT space, u0 in [0.1, 0.9], w perpendicular to tangent and ray, rho in
    [0, 0.9] or [1.1, 3] half and half, no nearer than 25 degrees to the tangent, from `distances`, |d| from `dlens`; taken to world space in float64 and rounded to
    fp32.  axes: the WORLD direction is exactly +-x, +-y or +-z (the other components +0.0 or -0.0), the origin placed so that the ray goes through the target."""
    rs = np.random.RandomState(seed)
    insts = R.curve_instances(arr)
    rays = np.zeros(n, S.RAY)
    for i in range(n):
        _, Mx, segs, _ = insts[rs.randint(len(insts))]
        q = segs[rs.randint(len(segs))]
        u0 = rs.uniform(0.1, 0.9)
        c, c1 = bspline(q, u0), bspline(q, u0, 1)
        tan = c1[:3] / np.linalg.norm(c1[:3])
        Mi = np.linalg.inv(Mx[:, :3])
        while True:
            if axes:
                vw = np.zeros(3)
                vw[rs.randint(3)] = rs.choice([-1.0, 1.0])
                v = Mi @ vw
                v /= np.linalg.norm(v)
                if abs(v @ tan) >= np.cos(np.radians(25.0)):  # (another segment, another axis)
                    q = segs[rs.randint(len(segs))]
                    c, c1 = bspline(q, u0), bspline(q, u0, 1)
                    tan = c1[:3] / np.linalg.norm(c1[:3])
                    continue
                break
            v = rs.normal(size=3)
            v /= np.linalg.norm(v)
            if abs(v @ tan) < np.cos(np.radians(25.0)):
                break
        w = np.cross(tan, v)
        w /= np.linalg.norm(w)
        rho = rs.uniform(0.0, 0.9) if i % 2 == 0 else rs.uniform(1.1, 3.0)
        target = Mx[:, :3] @ (c[:3] + rho * c[3] * w * rs.choice([-1.0, 1.0])) + Mx[:, 3]
        dw = Mx[:, :3] @ v
        dw /= np.linalg.norm(dw)
        ds, dl = rs.choice(distances), rs.choice(dlens)
        if axes:
            dw = np.where(vw == 0.0, rs.choice([0.0, -0.0], 3), vw)
        rays["origin"][i] = (target - dw * ds).astype(np.float32)
        if axes:
            rays["dir"][i] = dw.astype(np.float32)
        else:
            dd = target - rays["origin"][i].astype(np.float64)
            rays["dir"][i] = (dd / np.linalg.norm(dd) * dl).astype(np.float32)
    rays["tmin"], rays["tmax"] = 0.0, 1e16
    return rays


_CASES = {}


def case(name, build):
    """(arr, rays, float64 reference) of a named case, made once"""
    if name not in _CASES:
        arr, rays = build()
        _CASES[name] = (arr, rays, R.trace(arr, rays))
    return _CASES[name]


def patch_case(xf, n=1500, axes=False, seed=3):
    def build():
        pts, rad = strands(21)
        arr = make_scene(pts, rad, XF[xf])
        return arr, aim(arr, n, seed, axes=axes)

    return case(("patch", xf, n, axes, seed), build)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the judgement
# ---------------------------------------------------------------------------------------------------------------------------------------------
def dlen(rays):
    return np.linalg.norm(rays["dir"].astype(np.float64), axis=1)


def hold_closest(what, rays, hits, ref, min_hits=100, min_misses=100, allow_inside=False, same_prim=True):
    """closest-hit records against the reference: the decision on every decided ray, t, u and the surface distance within their bars, the instance and segment named"""
    got = hits["instance_id"] != MISS
    j = R.judge(ref, got, hits["t"], hits["u"], dlen(rays), ref["world_scale"], ref["kappa"], allow_inside=allow_inside)
    dec = j["decided"]
    both = dec & ref["hit"] & got
    if not same_prim:  # (overlapping tubes: where two surfaces cross, which one the entry belongs to is not decided; u and the surface are judged on the rays that name the same one)
        same = (hits["prim_id"] == ref["seg"]) & (hits["instance_id"] == ref["inst"])
        j["ru"], j["rs"] = np.where(same, j["ru"], np.nan), np.where(same, j["rs"], np.nan)
    worst = {k: float(np.nanmax(j[k][both])) if both.any() and np.isfinite(j[k][both]).any() else 0.0 for k in ("rt", "ru", "rs")}
    print(f"{what}: {len(rays)} rays, {int(dec.sum())} decided ({int((dec & ref['hit']).sum())} hits), {int((dec & ~j['agree']).sum())} disagree, "
          f"worst |dt| / bar_t {worst['rt']:.3f}, |du| / bar_u {worst['ru']:.3f}, surface / bar_surf {worst['rs']:.3f}")
    LOG[what] = {"rays": len(rays), "decided": int(dec.sum()), "decided_hits": int((dec & ref["hit"]).sum()), "disagree": int((dec & ~j["agree"]).sum()), **worst}
    assert (dec & ref["hit"]).sum() >= min_hits and (dec & ~ref["hit"]).sum() >= min_misses, what
    bad = np.nonzero(dec & ~j["agree"])[0]
    assert not len(bad), (what, "decision", bad[:8], ref["depth"][bad[:8]], j["m"][bad[:8]])
    assert worst["rt"] <= 1.0 and worst["ru"] <= 1.0 and worst["rs"] <= 1.0, (what, worst)
    if same_prim:
        wrong = both & ((hits["prim_id"] != ref["seg"]) | (hits["instance_id"] != ref["inst"]))
        assert not wrong.any(), (what, "names", np.nonzero(wrong)[0][:8])
    return j


def bar_t_of(ref, j, k):
    """bar_t of the decided hits k, in units of the ray's own parameter"""
    return R.t_bar(ref["distance"][k], ref["radius"][k], ref["speed"][k], ref["bend"][k], np.linalg.norm(ref["cps"][k][:, :, :3] - ref["cps"][k][:, :, :3].mean(axis=1, keepdims=True), axis=2).max(axis=1),
                   ref["angle"][k], 1.0 + ref["depth"][k], ref["world_scale"][k], ref["kappa"][k])


def hold_any_hit(what, trace, rays, ref, j):
    """any-hit (mode 1): with tmax 4 bar_t before the entry the ray is free, 4 bar_t after it occluded; a decided miss is free at any tmax"""
    k = j["decided"] & ref["hit"]
    step = np.zeros(len(rays))
    step[k] = 4.0 * bar_t_of(ref, j, k) / dlen(rays)[k]
    before, after = rays.copy(), rays.copy()
    before["tmax"] = np.where(k, np.nextafter((ref["t"] - step).astype(np.float32), np.float32(0)), rays["tmax"])
    after["tmax"] = np.where(k, np.nextafter((ref["t"] + step).astype(np.float32), np.float32(np.inf)), rays["tmax"])
    hb, ha = trace(before, 1), trace(after, 1)
    free = j["decided"] & (hb["t"] > 0)
    assert not free.any(), (what, "occluded before the entry", np.nonzero(free)[0][:8])
    blocked = k & ~(ha["t"] > 0)
    assert not blocked.any(), (what, "free after the entry", np.nonzero(blocked)[0][:8])
    return before, after


def equal_to_checker(arr, queries):
    """the checker's records for the same queries, bit for bit (as tests/test_gpu_parity.py holds them): after the float64 judgement, so that a failure here alone says
    the two compilations of the shared text parted, and one above alone that both are wrong together"""
    from tests import orklib

    o = orklib.new_context()
    o.set_scene(arr)
    for rays, mode, hits in queries:
        want = o.trace(rays, mode)
        if mode == 1:
            assert np.array_equal(hits["t"], want["t"])
            continue
        for f in ("instance_id", "prim_id"):
            assert np.array_equal(hits[f], want[f]), f
        for f in ("t", "u", "v"):
            assert np.array_equal(hits[f].view(np.uint32), want[f].view(np.uint32)), f


LOG = {}


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    R.record("device", LOG)


def device(arr, **options):
    from strelka_amd import capi

    ctx = capi.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_scene(arr)
    return ctx


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xf", ["identity", "rotated_scaled"])
@pytest.mark.parametrize("split", [1, 2, 5, 8])
def test_sub_range_counts_against_float64(split, xf):
    arr, rays, ref = patch_case(xf)
    ctx = device(arr, curve_split=split)
    hits = ctx.trace(rays, 0)
    hold_closest(f"split{split}_{xf}", rays, hits, ref)
    equal_to_checker(arr, [(rays, 0, hits)])
    ctx.close()


@pytest.mark.parametrize("xf", list(XF))
def test_instance_transforms_closest_and_any_hit_against_float64(xf):
    arr, rays, ref = patch_case(xf)
    ctx = device(arr)
    hits = ctx.trace(rays, 0)
    j = hold_closest(f"xf_{xf}", rays, hits, ref)
    before, after = hold_any_hit(f"xf_{xf}", ctx.trace, rays, ref, j)
    equal_to_checker(arr, [(rays, 0, hits), (before, 1, ctx.trace(before, 1)), (after, 1, ctx.trace(after, 1))])
    ctx.close()


def bundle_case():
    def build():
        pts, rad = bundle(8)
        arr = make_scene(pts, rad, XF["identity"])
        # 8 lines of 64 parallel rays: the origins of a line 1e-3 apart along the bundle's axis, so that a whole wave meets the 40 hairs at once;
        # a line crosses at a random angle >= 30 degrees and aims at a random offset within +-4 radii of the bundle's middle
        rs = np.random.RandomState(4)
        q = R.curve_instances(arr)[0][2]
        rays = np.zeros(8 * 64, S.RAY)
        for ln in range(8):
            s = rs.randint(1, 4)
            c, c1 = bspline(q[s], 0.3), bspline(q[s], 0.3, 1)
            tan = c1[:3] / np.linalg.norm(c1[:3])
            while True:
                v = rs.normal(size=3)
                v /= np.linalg.norm(v)
                if abs(v @ tan) < np.cos(np.radians(30.0)):
                    break
            w = np.cross(tan, v)
            w /= np.linalg.norm(w)
            for k in range(64):
                target = c[:3] + tan * 1e-3 * (k - 32) + w * rs.uniform(-4.0, 4.0) * 2e-4
                i = ln * 64 + k
                rays["origin"][i] = (target - v * 0.3).astype(np.float32)
                rays["dir"][i] = v.astype(np.float32)
        rays["tmin"], rays["tmax"] = 0.0, 1e16
        return arr, rays

    return case("bundle", build)


def test_forty_hairs_within_three_radii_met_by_whole_waves():
    arr, rays, ref = bundle_case()
    ctx = device(arr)
    hits = ctx.trace(rays, 0)
    hold_closest("bundle", rays, hits, ref, min_hits=100, min_misses=20, same_prim=False)
    equal_to_checker(arr, [(rays, 0, hits)])
    ctx.close()


def test_tmin_just_below_and_just_above_the_first_entry():
    """tmin 4 bar_t below the entry: the same entry.  4 bar_t above it: the next strand of the bundle the ray is not already inside, or a miss -- whatever the
    float64 reference says for that tmin."""
    arr, rays, ref = bundle_case()
    ctx = device(arr)
    j = R.judge(ref, ref["hit"], ref["t"], ref["u_foot"], dlen(rays), ref["world_scale"], ref["kappa"])
    k = j["decided"] & ref["hit"]
    assert k.sum() >= 100
    step = np.zeros(len(rays))
    step[k] = 4.0 * bar_t_of(ref, j, k) / dlen(rays)[k]
    below, above = rays[k].copy(), rays[k].copy()
    below["tmin"] = np.nextafter((ref["t"] - step)[k].astype(np.float32), np.float32(0))
    above["tmin"] = np.nextafter((ref["t"] + step)[k].astype(np.float32), np.float32(np.inf))
    hb = ctx.trace(below, 0)
    ref_b = {key: v[k] for key, v in ref.items()}
    hold_closest("tmin_below", below, hb, ref_b, min_hits=100, min_misses=0, same_prim=False)
    ref_a = case("bundle_above", lambda: (arr, above))[2]
    ha = ctx.trace(above, 0)
    hold_closest("tmin_above", above, ha, ref_a, min_hits=20, min_misses=0, allow_inside=True, same_prim=False)
    equal_to_checker(arr, [(below, 0, hb), (above, 0, ha)])
    ctx.close()


@pytest.mark.parametrize("xf", ["identity", "rotated_scaled"])
def test_rays_along_the_axes_with_signed_zeros(xf):
    arr, rays, ref = patch_case(xf, n=1200, axes=True, seed=6)
    d = rays["dir"]
    assert ((d != 0).sum(axis=1) == 1).all() and np.signbit(d[d == 0]).any() and (~np.signbit(d[d == 0])).any()
    ctx = device(arr)
    hits = ctx.trace(rays, 0)
    hold_closest(f"axes_{xf}", rays, hits, ref)
    equal_to_checker(arr, [(rays, 0, hits)])
    ctx.close()


def test_a_hair_wins_over_the_scalp_two_radii_behind_it():
    """strands lying in the plane z = 0.1 (crossing x and y obliquely), a quad at z = 0.1 - 2 r behind them, rays straight down -z from 0.3 above: a decided hit reports
    the hair (its entry lies 2 r ... 3 r in front of the quad), a decided miss the quad at t = 0.3 + 2 r."""
    r = 2e-4

    def build():
        pts, rad = strands(31)
        pts = pts.copy()
        pts[:, :, 2] = 0.1
        rad = np.full_like(rad, r)
        arr = make_scene(pts, rad, XF["identity"], mesh_z=np.float32(0.1) - np.float32(2 * r))
        rs = np.random.RandomState(9)
        q = R.curve_instances(arr)[0][2]
        n = 1500
        rays = np.zeros(n, S.RAY)
        for i in range(n):
            s, u0 = rs.randint(len(q)), rs.uniform(0.1, 0.9)
            c, c1 = bspline(q[s], u0), bspline(q[s], u0, 1)
            w = np.cross(c1[:3] / np.linalg.norm(c1[:3]), [0.0, 0.0, 1.0])
            rho = rs.uniform(0.0, 0.9) if i % 2 == 0 else rs.uniform(1.1, 3.0)
            target = c[:3] + w / np.linalg.norm(w) * rho * r * rs.choice([-1.0, 1.0])
            rays["origin"][i] = (target[0], target[1], 0.4)
        rays["dir"] = (0.0, 0.0, -1.0)
        rays["tmin"], rays["tmax"] = 0.0, 1e16
        return arr, rays

    arr, rays, ref = case("scalp", build)
    ctx = device(arr)
    hits = ctx.trace(rays, 0)
    curve_inst = int(np.nonzero(arr["instances"]["type"] == S.INSTANCE_CURVE)[0][0])
    mesh_inst = int(np.nonzero(arr["instances"]["type"] == S.INSTANCE_MESH)[0][0])
    on_curve = hits["instance_id"] == curve_inst
    got = hits.copy()
    got["instance_id"] = np.where(on_curve, hits["instance_id"], MISS)  # (for the curve's judgement the quad is a miss)
    j = hold_closest("scalp", rays, got, ref)
    behind = j["decided"] & ~ref["hit"]
    assert (hits["instance_id"][behind] == mesh_inst).all()
    plane_t = np.float64(np.float32(0.4)) - np.float64(np.float32(0.1) - np.float32(2 * r))
    assert np.abs(hits["t"][behind] - plane_t).max() <= 8 * R.U * 0.4
    gap = plane_t - ref["t"][j["decided"] & ref["hit"]]
    assert gap.min() >= 2 * r * 0.999 and gap.max() <= 3 * r * 1.001
    equal_to_checker(arr, [(rays, 0, hits)])
    ctx.close()


def test_grazing_hits_on_straight_strands_survive_the_cull():
    """The bounding cylinder of a sub-range is (its Bezier points' distance from their chord + the largest radius) 1.001 wide -- twice the radius with curve_split > 1 --, so
    on a bent hair it is far looser than the tube and a cull that is a little too tight hides in the slack.  Straight strands of constant radius leave none with
    curve_split = 1: rays that pass the axis at 0.95 r ... (1 - 1.1 m) r -- decided hits, by float64 -- must all be found."""
    r = 4e-4

    def build():
        rs = np.random.RandomState(12)
        n, n_cp = 64, 8
        p0 = rs.uniform(-0.12, 0.12, (n, 3))
        dr = rs.normal(size=(n, 3))
        dr /= np.linalg.norm(dr, axis=1, keepdims=True)
        pts = (p0[:, None, :] + dr[:, None, :] * (0.03 * np.arange(n_cp))[None, :, None]).astype(np.float32)
        arr = make_scene(pts, np.full((n, n_cp), r, np.float32), XF["identity"])
        q = R.curve_instances(arr)[0][2]
        m = float(R.margin(0.3, r, 0.03, 0.06))
        assert m < 0.02
        rays = np.zeros(1500, S.RAY)
        for i in range(len(rays)):
            s, u0 = rs.randint(len(q)), rs.uniform(0.1, 0.9)
            c, c1 = bspline(q[s], u0), bspline(q[s], u0, 1)
            tan = c1[:3] / np.linalg.norm(c1[:3])
            while True:
                v = rs.normal(size=3)
                v /= np.linalg.norm(v)
                if abs(v @ tan) < np.cos(np.radians(25.0)):
                    break
            w = np.cross(tan, v)
            w /= np.linalg.norm(w)
            rho = rs.uniform(0.95, 1.0 - 1.1 * m) if i % 4 else rs.uniform(1.0 + 1.1 * m, 1.05)
            target = c[:3] + rho * r * w * rs.choice([-1.0, 1.0])
            rays["origin"][i] = (target - v * 0.3).astype(np.float32)
            dd = target - rays["origin"][i].astype(np.float64)
            rays["dir"][i] = (dd / np.linalg.norm(dd)).astype(np.float32)
        rays["tmin"], rays["tmax"] = 0.0, 1e16
        return arr, rays

    arr, rays, ref = case("straight", build)
    ctx = device(arr, curve_split=1)
    hits = ctx.trace(rays, 0)
    j = hold_closest("straight_grazing", rays, hits, ref, min_hits=600, min_misses=200)
    grazing = j["decided"] & ref["hit"] & (ref["depth"] > -0.015)  # (the outermost 1.5 % of the radius)
    assert grazing.sum() >= 100
    equal_to_checker(arr, [(rays, 0, hits)])
    ctx.close()
