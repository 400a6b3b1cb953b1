"""tests/furnaceref.py against itself ("The integrator against the furnace"): the closed form expected() against the float64 random walk
that restates the loop it was derived from, the last-vertex share, the variance bounds against the walk's sample variances in every case
tests/test_gpu_furnace.py uses, and the condition under which the throughput cut never fires.  No GPU, no library code on the checked side."""
import numpy as np
import pytest

from strelka_amd import scene as S
from tests import furnaceref as F
from tests import test_gpu_furnace as G

LE = G.f64(G.LE)
N_WALK = 1 << 16


def rays(n, seed):
    sc = G.room((0.5, 0.5, 0.5))
    p = S.frame_params(sc.getCamera(), G.STAT_W, G.STAT_W)
    rng = np.random.default_rng(seed)
    o, d = F.camera_rays(p["view_to_world"], p["clip_to_view"], n, rng)
    return o, d, rng


def test_camera_rays_start_inside_and_span_the_field_of_view():
    o, d, _ = rays(4096, 1)
    assert (np.abs(o) < 1).all() and np.linalg.norm(G.EYE) > G.SPHERE_R + 0.1 and np.allclose(o, G.EYE, atol=1e-6) and np.allclose(np.linalg.norm(d, axis=1), 1)
    axis = np.subtract(G.AT, G.EYE) / np.linalg.norm(np.subtract(G.AT, G.EYE))
    c = d @ axis
    half = np.radians(G.FOV / 2)
    assert c.min() > np.cos(np.arctan(np.sqrt(2) * np.tan(half))) - 1e-6 and c.max() > np.cos(0.02)


@pytest.mark.parametrize("rho", [tuple(G.RHO_COLOUR), (0.5, 0.5, 0.5)])
def test_walk_without_nee_is_expected_exactly_up_to_depth_5(rho):
    """no random number reaches the value: every path returns expected()'s float64 bits"""
    r = G.f64(rho)
    for d in (1, 2, 3, 4, 5):
        o, dirs, rng = rays(512, d)
        w = F.walk(LE, r, d, o, dirs, rng)
        mu = F.expected(LE, r, d)
        assert np.array_equal(w["L"], np.broadcast_to(mu, w["L"].shape)) and (w["M"] == d).all() and w["cuts"] == 0
        assert np.allclose(mu, sum(LE * r ** k for k in range(d)), rtol=1e-15)
        assert np.allclose(F.nee_reach(LE, r, d), LE * r ** d, rtol=1e-15)


@pytest.mark.parametrize("rho", [0.5, 0.8])
@pytest.mark.parametrize("d", [8, 32])
def test_walk_without_nee_agrees_with_expected_beyond_the_roulette(rho, d):
    r = G.f64(np.full(3, rho, np.float32))
    o, dirs, rng = rays(N_WALK, 10 * d)
    w = F.walk(LE, r, d, o, dirs, rng)
    mu, mean = F.expected(LE, r, d), w["L"].mean(0)
    se = w["L"].std(0, ddof=1) / np.sqrt(N_WALK)
    print(f"rho {rho} depth {d}: mean {mean}, expected {mu}, |diff| / 6 se {np.abs(mean - mu) / (6 * se)}")
    assert (np.abs(mean - mu) <= 6 * se).all() and w["cuts"] == 0
    # ... and with what the loop's quirks cost against the plain series: p / (p + 1e-5) per roulette step, the remainder beyond the depth limit
    full = F.l_inf(LE, r) * (1 - r ** d)
    assert (mu < full).all() and (mu > full * (1 - 1e-3)).all()


@pytest.mark.parametrize("rho,num_pick", [(0.5, 1), (0.8, 1), (0.5, 2)])
def test_walk_with_nee_returns_to_the_full_series(rho, num_pick):
    """max_depth 64: the truncated remainder is below rho^64, the roulette's 1e-5 takes < 1e-3 of it (well inside 6 se here); MIS with the balance heuristic,
    whatever 1 / num_pick, neither loses nor gains"""
    r = G.f64(np.full(3, rho, np.float32))
    o, dirs, rng = rays(N_WALK, 77)
    w = F.walk(LE, r, 64, o, dirs, rng, nee=True, num_pick=num_pick)
    mean, se = w["L"].mean(0), w["L"].std(0, ddof=1) / np.sqrt(N_WALK)
    print(f"rho {rho} num_pick {num_pick}: mean {mean}, L_inf {F.l_inf(LE, r)}, |diff| / 6 se {np.abs(mean - F.l_inf(LE, r)) / (6 * se)}, 6 se / L_inf {6 * se / F.l_inf(LE, r)}")
    assert (np.abs(mean - F.l_inf(LE, r)) <= 6 * se).all() and (6 * se <= 0.05 * F.l_inf(LE, r)).all()


@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_nee_adds_the_last_vertex_share_and_nothing_else(d):
    """NEE on agrees with NEE off except for the vertex no BSDF hit gathers: mean = expected() + nee_reach() s_d, s_d in (0, 1) measured on the same paths"""
    r = G.f64(G.RHO_COLOUR)
    o, dirs, rng = rays(N_WALK, 5 + d)
    s, se_s, w = F.last_vertex_share(LE, r, d, o, dirs, rng)
    mean, se = w["L"].mean(0), w["L"].std(0, ddof=1) / np.sqrt(N_WALK)
    mu = F.expected(LE, r, d) + F.nee_reach(LE, r, d) * s
    print(f"depth {d}: s_d {s:.4f} +- {se_s:.4f}, mean {mean}, mu {mu}, |diff| / 6 se {np.abs(mean - mu) / (6 * se)}")
    assert 0.2 < s < 0.8 and se_s < 0.01
    assert (np.abs(mean - mu) <= 6 * se).all()
    assert (np.abs(mean - F.expected(LE, r, d)) > 6 * se).any() or d > 3  # (the share is there to be seen)


def test_the_variance_bounds_bound_the_walk_in_every_gpu_case():
    n = N_WALK
    for rho, mode in G.DEEP:
        r = G.f64(np.full(3, rho, np.float32))
        o, dirs, rng = rays(n, 3)
        nee = mode != "nee_off"
        w = F.walk(LE, r, 32, o, dirs, rng, nee=nee, num_pick=2 if mode.endswith("below") else 1)
        mu, _, V, N = G.deep_case(rho, mode)
        var = w["L"].var(0, ddof=1)
        print(f"deep rho {rho} {mode}: sample variance {var}, bound {V}, N {N}")
        # the sample variance of n paths scatters by about sqrt(kurtosis / n) of itself: 10 % is generous for 2^17; NEE off the bound IS the variance
        assert (var <= V * 1.1).all() and (V > 0).all()
        if not nee:
            assert (np.abs(var / V - 1) < 0.1).all()
        # a room with objects: the bound that knows nothing of the order of walls and objects is the weaker one
        assert (F.variance_bound_objects(LE, r, nee, mu * 0) >= V).all()
    for d in (1, 2, 3):
        r = G.f64(G.RHO_COLOUR)
        o, dirs, rng = rays(n, 4)
        w = F.walk(LE, r, d, o, dirs, rng, nee=True)
        mu = w["L"].mean(0)
        V = F.variance_bound(LE, r, d, True, mu)
        assert (w["L"].var(0, ddof=1) <= V).all()
        assert (w["L"] <= np.cumsum([LE * r ** k * (1 + r) for k in range(d)], 0)[-1] * (1 + 1e-12)).all()  # B(M) pointwise


def test_sample_counts_stay_small():
    """what the GPU file will launch: P N <= 2^23 everywhere, the deep bars under 1 % of mu"""
    for rho, mode in G.DEEP:
        mu, hi, V, N = G.deep_case(rho, mode)
        bar = 6 * np.sqrt(V / (G.STAT_W ** 2 * N)) + G.eps(N) * mu
        print(f"deep rho {rho} {mode}: N {N}, bar / mu {bar / mu}")
        assert (bar <= 0.01 * mu).all() and G.STAT_W ** 2 * N <= 2 ** 23
    for obj, depth, per_wall, two_sided in G.OBJECTS:
        for nee in (False, True):
            lo, hi, bar, N = G.object_case(obj, depth, per_wall, two_sided, nee)
            print(f"{obj} nee {nee}: N {N}, bar / L_inf {bar / hi}, bracket width / bar {(hi - lo) / bar}")
            assert (bar <= 0.02 * hi).all() and G.STAT_W ** 2 * N <= 2 ** 23 and (not two_sided or (hi - lo <= 1e-3 * bar).all())


def test_the_cut_never_fires_for_the_inputs():
    for rho in (G.RHO_COLOUR, np.float32([0.5] * 3), np.float32([0.8] * 3), np.float32([G.OBJ_RHO] * 3)):
        assert F.no_cut_condition(G.f64(rho))
        T, S = F.loop(G.f64(rho), 64)
        assert ((T * T).sum(1) >= 2 * F.CUT).all()  # with the factor 2 the condition keeps for the device's fp32
    assert F.no_cut_condition([0.3, 0.3, 0.3]) and not F.no_cut_condition([0.2, 0.2, 0.2]) and not F.no_cut_condition([0.24, 0.1, 0.1])
    with pytest.raises(AssertionError):
        F.expected(LE, [0.1, 0.1, 0.1], 8)
    # a room where it does fire is not the closed form's: the walk says so
    o, dirs, rng = rays(256, 9)
    assert F.walk(LE, np.full(3, 0.2), 6, o, dirs, rng)["cuts"] > 0


def test_the_room_is_closed_and_wound_inwards():
    for kw in ({}, {"instanced": True, "xf": G.ROOM_XF}):
        arr = G.room(tuple(G.RHO_COLOUR), **kw).arrays()
        tris = []
        for inst in arr["instances"]:
            m = arr["meshes"][inst["geom_id"]]
            v = arr["vertices"]["pos"][int(m["vertex_offset"]):int(m["vertex_offset"]) + int(m["vertex_count"])].astype(np.float64)
            M = np.vstack([np.asarray(inst["transform"], np.float64).reshape(3, 4), [0, 0, 0, 1]])
            tris.append((v @ M[:3, :3].T + M[:3, 3]).reshape(-1, 3, 3))
        tris = np.concatenate(tris)
        xf = kw.get("xf", np.eye(4))
        centre = (xf @ [0, 0, 0, 1.0])[:3]
        n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
        assert len(tris) == 12 and ((n * (centre - tris[:, 0])).sum(1) > 0).all()  # every front side faces the centre
        # closed: the signed volume of the 12 triangles is minus the box's (inward winding), 8 det(xf)
        vol = (tris[:, 0] * np.cross(tris[:, 1], tris[:, 2])).sum() / 6.0
        assert abs(vol + 8.0 * np.linalg.det(xf[:3, :3])) < 1e-5
    s = G.sphere_triangles(G.SPHERE_R)
    vol = (s[:, 0].astype(np.float64) * np.cross(s[:, 1].astype(np.float64), s[:, 2].astype(np.float64))).sum() / 6.0
    assert 0.85 * 4 / 3 * np.pi * G.SPHERE_R ** 3 < vol < 4 / 3 * np.pi * G.SPHERE_R ** 3  # outward winding, closed (an open or mixed winding has no such volume)
    edges = {}
    for t in s:
        for a, b in ((0, 1), (1, 2), (2, 0)):
            k = (t[a].tobytes(), t[b].tobytes())
            edges[k] = edges.get(k, 0) + 1
    assert all(v == 1 and (k[1], k[0]) in edges for k, v in edges.items())  # every edge once in each direction: watertight, vertices bit-identical
