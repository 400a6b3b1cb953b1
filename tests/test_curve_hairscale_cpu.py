"""The checker's round cubic B-spline intersector at HAIR scale against float64 ("Curve intersection against float64").

tests/curveref.py states the primitive from its definition -- the first entry of the ray into the union of the spheres (C(u), r(u)) -- and the bounds an fp32
intersector is held to: written-out counts of roundings, relative to the tube's radius and the distance, never an absolute figure.  Here `ork_intersect_curve` and
the checker's scene trace are held to it over r in {4e-4, 1e-4, 2e-5} x segment length in {0.03, 0.12} x distance in {0.3, 3, 30, 300} x |d| in {1, 37, 1 / 37}, and
over strands that taper 4 : 1 along the segment.  tests/test_gpu_curve_hairscale.py runs the device through the same judge.

Only rays float64 DECIDES are judged (curveref.judge): the origin outside, the line clear of or inside every tube by the margin m = curveref.margin, a hit entering at u in
[0.03, 0.97] at 20 degrees or more to the tangent.  A cell whose nominal m exceeds 0.5 is skipped BY NAME (the list is printed, written with the measured figures to curve_hairscale.json in the directory SKH_MEASURED_DIR names, and asserted to be what the rule
says and to stay within the distance-300 column and r = 2e-5 at distance 30); in every other cell 60 % of the generated rays must be decided.

The injected errors the two files were shown to catch (each applied to a scratch copy of the checker's / the device's text, never committed) are listed in
tests/test_gpu_curve_hairscale.py's docstring."""
import ctypes as C
import itertools

import numpy as np
import pytest

from strelka_amd import scene as S
from tests import curveref as R
from tests import orklib
from tests.hitref import bspline

RADII = (4e-4, 1e-4, 2e-5)
LENGTHS = (0.03, 0.12)
DISTANCES = (0.3, 3.0, 30.0, 300.0)
DLENS = (1.0, 37.0, 1.0 / 37.0)
RAYS_PER_CELL = 96


def cells():
    """(name, r, length, distance, |d|, tapering): the grid, and the tapering strands at |d| = 1 up to distance 30"""
    out = [(f"r{r:g}_len{ln:g}_dist{ds:g}_d{dl:.3g}", r, ln, ds, dl, False) for r, ln, ds, dl in itertools.product(RADII, LENGTHS, DISTANCES, DLENS)]
    out += [(f"taper_r{r:g}_len{ln:g}_dist{ds:g}", r, ln, ds, 1.0, True) for r, ln, ds in itertools.product(RADII, LENGTHS, DISTANCES[:3])]
    return out


def nominal_margin(r, ln, ds, taper):
    """the cell's m from its nominal figures: the distance, |C'| = the spacing of the control points, the smallest radius of the segment (a tapering strand:
    2 r at u = 1, see segment())"""
    return float(R.margin(ds, r * (2.0 if taper else 1.0), ln, 2.0 * ln))


def segment(rs, r, ln, taper, centre):
    """four control points `ln` apart along a gently bent line (the hair stand-in's strands bend by a few degrees per segment), radius r -- or control radii 4 r, 3 r, 2 r, r
    towards the tip for a tapering strand: the segment's own radius runs from 3 r to 2 r"""
    step = np.array([1.0, 0.0, 0.0]) + rs.normal(size=3) * 0.1
    rot = np.linalg.qr(rs.normal(size=(3, 3)))[0]
    pts = [np.zeros(3)]
    for _ in range(3):
        step = step + rs.normal(size=3) * 0.12
        step /= np.linalg.norm(step)
        pts.append(pts[-1] + step * ln)
    pts = (np.array(pts) - np.mean(pts, axis=0)) @ rot.T + centre
    rad = r * (np.array([4.0, 3.0, 2.0, 1.0]) if taper else np.ones(4))
    return np.concatenate([pts, rad[:, None]], 1).astype(np.float32)


def aim(rs, q, ds, dl, m, n):
    """n rays at segment q from distance ds: through C(u0) + rho r(u0) w, u0 in [0.1, 0.9], w perpendicular to both the tangent and the ray -- so the line passes the
    (locally straight) axis at rho r --, half of them rho in [0, 1 - 1.25 m) (hits), half in (1 + 1.25 m, 3] (misses); directions no nearer than 25 degrees to the
    tangent (the tangent case has its own test, tests/test_oracle_intersect.py); the direction scaled to |d| = dl and rounded to fp32, as the origin is"""
    q64 = q.astype(np.float64)
    o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for i in range(n):
        u0 = rs.uniform(0.1, 0.9)
        c, c1 = bspline(q64, u0), bspline(q64, u0, 1)
        tan = c1[:3] / np.linalg.norm(c1[:3])
        while True:
            v = rs.normal(size=3)
            v /= np.linalg.norm(v)
            if abs(v @ tan) < np.cos(np.radians(25.0)):
                break
        w = np.cross(tan, v)
        w /= np.linalg.norm(w)
        rho = rs.uniform(0.0, 1.0 - 1.25 * m) if i % 2 == 0 else rs.uniform(1.0 + 1.25 * m, 3.0)
        target = c[:3] + rho * c[3] * w * rs.choice([-1.0, 1.0])
        o[i] = (target - v * ds).astype(np.float32)
        dd = target - o[i].astype(np.float64)
        d[i] = (dd / np.linalg.norm(dd) * dl).astype(np.float32)
    return o, d


_GRID = None


def grid():
    """every cell's segment (on a lattice 2 apart, so that no ray aimed at one comes near another's by more than chance) and rays, and the float64 reference of
    each ray against its own segment; computed once"""
    global _GRID
    if _GRID is None:
        rs = np.random.RandomState(2024)
        cs = cells()
        segs, O, D, cell_of, skipped = [], [], [], [], []
        for k, (name, r, ln, ds, dl, taper) in enumerate(cs):
            centre = np.array([k % 10, (k // 10) % 10, 0.0]) * 2.0 - np.array([9.0, 8.0, 0.0])
            q = segment(rs, r, ln, taper, centre)
            segs.append(q)
            m = nominal_margin(r, ln, ds, taper)
            if m > R.M_CAP:
                skipped.append(name)
                continue
            o, d = aim(rs, q, ds, dl, m, RAYS_PER_CELL)
            O.append(o), D.append(d), cell_of.append(np.full(len(o), k))
        segs = np.array(segs)
        O, D, cell_of = np.concatenate(O), np.concatenate(D), np.concatenate(cell_of)
        ref = R.first_entry(O, D, segs, only=cell_of)
        _GRID = {"cells": cs, "segs": segs, "o": O, "d": D, "cell": cell_of, "skipped": skipped, "ref": ref, "dlen": np.linalg.norm(D.astype(np.float64), axis=1)}
    return _GRID


def summarise(g, j, what, require_share=True):
    """per cell: the decided share, the agreement, the worst t, u and surface errors as multiples of their bars -> rows; asserts the issue's conditions"""
    rows, bad = {}, []
    for k, (name, *_rest) in enumerate(g["cells"]):
        sel = g["cell"] == k
        if not sel.any():
            continue
        dec = sel & j["decided"]
        hits = dec & g["ref"]["hit"]
        row = {"rays": int(sel.sum()), "decided": int(dec.sum()), "decided_hits": int(hits.sum()), "disagree": int((dec & ~j["agree"]).sum())}
        for key in ("rt", "ru", "rs"):
            v = j[key][hits]
            row[key] = float(np.nanmax(v)) if np.isfinite(v).any() else 0.0
        rows[name] = row
        if require_share and row["decided"] < 0.6 * row["rays"]:
            bad.append((name, "decided share", row))
        if row["disagree"] or max(row["rt"], row["ru"], row["rs"]) > 1.0:
            bad.append((name, "bar", row))
    worst = {key: max(r[key] for r in rows.values()) for key in ("rt", "ru", "rs")}
    print(f"{what}: {len(rows)} cells, {sum(r['decided'] for r in rows.values())} decided rays, worst |dt| / bar_t {worst['rt']:.3f}, |du| / bar_u {worst['ru']:.3f}, surface / bar_surf {worst['rs']:.3f}")
    R.record(what, {"skipped_cells": g["skipped"], "worst": worst, "cells": rows})
    assert not bad, bad[:6]
    return rows


def test_reference_agrees_with_the_dense_scan():
    """curveref against the dense scan of tests/test_oracle_intersect.py::test_curve_intersector_finds_the_first_entry_into_the_swept_volume on that test's thick
    segment and rays (1 501 ray steps x 501 spheres for the bracket; the bracket bisected 50 times, the depth's minimum over u polished by a golden-section search so that the scan
    speaks of the same continuous family of spheres): the same rays hit, and t agrees to 1e-9 (measured 6e-15)."""
    rs = np.random.RandomState(11)
    q = np.array([0, 0, 0, 0.05, 1, 0.3, 0, 0.06, 2, -0.2, 0.4, 0.04, 3, 0, 0, 0.03], np.float32).reshape(1, 4, 4).astype(np.float64)
    us = np.linspace(0.0, 1.0, 501)  # (enough for the bracket: the spheres are 2e-3 apart, a fifteenth of the smallest radius; the bisection's depth is continuous in u)
    CU = bspline(q, us)

    def depth(P, polish):
        dist = np.linalg.norm(P[:, None, :] - CU[None, :, :3], axis=2) - CU[None, :, 3]
        if not polish:
            return dist.min(axis=1)
        j = dist.argmin(axis=1)
        lo, hi = us[np.maximum(j - 1, 0)], us[np.minimum(j + 1, len(us) - 1)]
        for _ in range(60):
            a, b = lo + (hi - lo) * 0.381966, lo + (hi - lo) * 0.618034
            ca, cb = bspline(q, a), bspline(q, b)
            left = np.linalg.norm(P - ca[:, :3], axis=1) - ca[:, 3] < np.linalg.norm(P - cb[:, :3], axis=1) - cb[:, 3]
            hi, lo = np.where(left, b, hi), np.where(left, lo, a)
        c = bspline(q, 0.5 * (lo + hi))
        return np.linalg.norm(P - c[:, :3], axis=1) - c[:, 3]

    O, D = [], []
    for _ in range(110):
        k = rs.randint(75, 425)
        c, r = CU[k, :3], CU[k, 3]
        off = rs.normal(size=3)
        off *= rs.choice([rs.uniform(0.0, 0.8), rs.uniform(1.6, 3.0)]) * r / np.linalg.norm(off)
        target = c + off
        o = (target + rs.normal(size=3) * 1.5).astype(np.float32)
        d = target - o.astype(np.float64)
        O.append(o.astype(np.float64)), D.append((d / np.linalg.norm(d)).astype(np.float32).astype(np.float64))
    O, D = np.array(O), np.array(D)
    ts = np.linspace(0.0, 6.0, 1501)
    dep = np.stack([depth(O[i][None, :] + ts[:, None] * D[i][None, :], False) for i in range(len(O))])  # (rays, steps)
    keep = (dep[:, 0] >= 0) & ((dep < 0).any(axis=1) | (dep.min(axis=1) > 1e-3))  # (origin outside; not a graze the scan's 1 501 steps cannot decide)
    O, D, dep = O[keep], D[keep], dep[keep]
    enters = (dep < 0).any(axis=1)
    first = np.argmax(dep < 0, axis=1)
    lo, hi = ts[np.maximum(first - 1, 0)], ts[first]
    for _ in range(50):  # (all rays at once)
        mid = 0.5 * (lo + hi)
        inside = depth(O + mid[:, None] * D, True) < 0
        hi, lo = np.where(inside, mid, hi), np.where(inside, lo, mid)
    T = np.where(enters, 0.5 * (lo + hi), np.nan)
    ref = R.first_entry(O, D, q)
    assert np.array_equal(ref["hit"], np.isfinite(T)) and ref["hit"].sum() > 60 and (~ref["hit"]).sum() > 20
    assert np.abs(ref["t"] - T)[ref["hit"]].max() < 1e-9
    # the record: a hit's depth is negative, a miss's positive; u names the sphere the entry lies on
    assert (ref["depth"][ref["hit"]] < 0).all() and (ref["depth"][~ref["hit"]] > 0).all()
    p = O[ref["hit"]] + ref["t"][ref["hit"], None] * D[ref["hit"]]
    c = bspline(q, ref["u"][ref["hit"]])
    assert np.abs(np.linalg.norm(p - c[:, :3], axis=1) - c[:, 3]).max() < 1e-12


def test_skipped_cells_are_the_ones_the_margin_rule_names():
    g = grid()
    print("skipped (nominal m > 0.5):", g["skipped"])
    for name in g["skipped"]:
        assert "_dist300" in name or ("r2e-05" in name and "_dist30" in name), name
    want = [name for name, r, ln, ds, dl, taper in g["cells"] if nominal_margin(r, ln, ds, taper) > R.M_CAP]
    assert g["skipped"] == want and len(g["skipped"]) < len(g["cells"]) // 3


def test_the_reference_alone_decides_enough_rays():
    """>= 60 % of every unskipped cell's rays are decided, before any intersector is asked: judged with an answer equal to the reference's"""
    g = grid()
    ref = g["ref"]
    j = R.judge(ref, ref["hit"], ref["t"], ref["u_foot"], g["dlen"])
    for k, (name, *_rest) in enumerate(g["cells"]):
        sel = g["cell"] == k
        if sel.any():
            assert j["decided"][sel].mean() >= 0.6, (name, j["decided"][sel].mean())
            assert (j["decided"] & ref["hit"])[sel].sum() >= 0.2 * sel.sum() and (j["decided"] & ~ref["hit"])[sel].sum() >= 0.2 * sel.sum(), name


def test_checker_intersector_against_float64_at_hair_scale(ork):
    g = grid()
    n = len(g["o"])
    hit, t, u = np.zeros(n, bool), np.zeros(n), np.zeros(n)
    out = np.zeros(2, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for i in range(n):
        o, d, q = np.ascontiguousarray(g["o"][i]), np.ascontiguousarray(g["d"][i]), np.ascontiguousarray(g["segs"][g["cell"][i]].reshape(16))
        hit[i] = bool(ork.ork_intersect_curve(p(o), p(d), 0.0, 1e16, p(q), p(out)))
        t[i], u[i] = out
    j = R.judge(g["ref"], hit, t, u, g["dlen"])
    summarise(g, j, "checker_intersector")


def grid_scene(matrix):
    """every cell's segment as a strand of four control points in ONE curve set under `matrix` (the control points taken to its object space in float64 first, then
    rounded: the object-space segments are what both sides are given), the grid's rays unchanged"""
    g = grid()
    Mi = np.linalg.inv(matrix)
    pts = g["segs"][:, :, :3].astype(np.float64).reshape(-1, 3) @ Mi[:3, :3].T + Mi[:3, 3]
    sc = S.Scene()
    mat = sc.addHairMaterial()
    cid = sc.createCurve(np.full(len(g["segs"]), 4, np.uint32), pts, g["segs"][:, :, 3].reshape(-1))
    sc.createInstance(S.INSTANCE_CURVE, cid, mat, matrix)
    rays = np.zeros(len(g["o"]), S.RAY)
    rays["origin"], rays["dir"], rays["tmin"], rays["tmax"] = g["o"], g["d"], 0.0, 1e16
    return sc.arrays(), rays


XFORMS = {"identity": np.eye(4), "rotated_scaled": S.translate((0.1, -0.2, 0.05)) @ S.rotate((0.3, 1.0, 0.2), 0.7) @ S.scale((1.3, 0.8, 1.1))}


def judge_scene(arr, rays, hits, identity):
    """a scene trace's hit records against curveref.trace"""
    ref = R.trace(arr, rays)
    got = hits["instance_id"] != 0xFFFFFFFF
    j = R.judge(ref, got, hits["t"], hits["u"], np.linalg.norm(rays["dir"].astype(np.float64), axis=1), 0.0 if identity else ref["world_scale"], ref["kappa"])
    right = ~(j["decided"] & ref["hit"] & got) | ((hits["prim_id"] == ref["seg"]) & (hits["instance_id"] == ref["inst"]))
    return ref, j, right


@pytest.mark.parametrize("xform", list(XFORMS))
def test_checker_scene_trace_against_float64_at_hair_scale(xform):
    """the same rays through the checker's hierarchy and instance transform (`ork_trace`); a decided hit names the reference's segment"""
    g = grid()
    arr, rays = grid_scene(XFORMS[xform])
    o = orklib.new_context()
    o.set_scene(arr)
    hits = o.trace(rays, 0)
    ref, j, right = judge_scene(arr, rays, hits, xform == "identity")
    assert right.all(), np.nonzero(~right)[0][:10]
    summarise(g, j, "checker_scene_" + xform, require_share=xform == "identity")
    assert j["decided"].mean() > 0.5
