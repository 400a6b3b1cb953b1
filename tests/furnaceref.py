"""The furnace: a closed room whose walls all have one Lambertian albedo rho and emit one radiance Le inwards ("The integrator against the
furnace").  The radiance in every direction at every point is Le sum rho^k whatever the room's shape, and lossless objects put into it change nothing; what the
renderer's bounce loop makes of it -- a depth limit, Russian roulette with its 1 / (p + 1e-5) rescale, the throughput cut, a last vertex that is never shaded -- is
written down here in float64, restated from the reference's loop (OptixRender.cu:118-154) and from DESIGN.md's definition of emissive meshes.  numpy only; nothing
is imported from the library or the checker.  tests/test_furnace_cpu.py holds this file against itself, tests/test_gpu_furnace.py the GPU against it.

The loop, per sample:  T = 1, depth = 0;  while depth < max_depth:  shade the vertex (it adds T Le w, then T *= rho for a Lambert sample: bsdf_over_pdf = base);
if depth > 3: p = max channel of T, stop if xi > p, else T *= 1 / (p + 1e-5);  stop if |T|^2 < 1e-5;  ++depth.
So vertices 0 .. max_depth - 1 are shaded, the roulette runs behind vertices 4, 5, ... (prd.depth is tested BEFORE its increment), a survivor's throughput is
T / (p + 1e-5) -- not T / p: each roulette step multiplies the expectation by p / (p + 1e-5) -- and the emission of vertex max_depth is never gathered by a BSDF hit."""
import numpy as np

RR_EPS = float(np.float32(1e-5))  # the loop's two constants as fp32 holds them
CUT = float(np.float32(1e-5))
RR_FROM = 4  # the first vertex behind which `prd.depth > 3` holds


def _c3(a):
    return np.array(np.broadcast_to(np.asarray(a, np.float64), (3,)))


def no_cut_condition(rho):
    """The cut `|T|^2 < 1e-5` never fires iff (i) behind vertices 0 .. 3, where T = rho^(k+1): sum_c rho_c^8 >= 1e-5 (the sum falls with k); (ii) behind a roulette,
    where the largest channel of T is p / (p + 1e-5): (p / (p + 1e-5))^2 >= 1e-5, i.e. p >= 3.2e-8.  p = rho_max^5 at the first roulette; if that is >= 1e-3 the
    survivor's largest channel is >= 0.99 and every later p >= 0.99 rho_max >= 0.99 * 1e-3^(1/5) = 0.25 by induction.  Sufficient, with a factor 2 on (i) for the
    device's fp32 evaluation: sum_c rho_c^8 >= 2e-5 and rho_max^5 >= 1e-3.  Every channel >= 0.3 gives 3 * 0.3^8 = 1.97e-4 and 0.3^5 = 2.4e-3.  White lossless
    objects in the room leave T alone and change neither."""
    rho = _c3(rho)
    return bool((rho ** 8).sum() >= 2 * CUT and rho.max() ** 5 >= 1e-3 and (rho < 1).all() and (rho > 0).all())


def loop(rho, max_depth):
    """The deterministic skeleton of a path in the room: T[k] = throughput at vertex k given the path is alive there, S[k] = the probability that it is
    (S[k+1] / S[k] = min(p_k, 1) behind vertices k >= 4), for k = 0 .. max_depth (the last entry belongs to the vertex that is never shaded)."""
    rho = _c3(rho)
    assert no_cut_condition(rho), rho
    T, S = [np.ones(3)], [1.0]
    for k in range(max_depth):
        t, s = T[-1] * rho, S[-1]
        if k >= RR_FROM:
            p = t.max()
            s = s * min(p, 1.0)
            t = t * (1.0 / (p + RR_EPS))
        assert t @ t >= CUT
        T.append(t), S.append(s)
    return np.array(T), np.array(S)


def expected(Le, rho, max_depth):
    """Expected radiance of one sample with emit_nee 0: sum over the shaded vertices of P(alive at k) T_k Le.  For max_depth <= 5 no random number reaches it."""
    Le = _c3(Le)
    T, S = loop(rho, max_depth)
    L = np.zeros(3)
    for k in range(max_depth):
        L = L + S[k] * (T[k] * Le)
    return L


def nee_reach(Le, rho, max_depth):
    """What the emitter NEE of the LAST shaded vertex could collect at most: P(alive) T_(d-1) rho Le = Le rho^d g, g the roulette factors up to vertex d - 1 (the
    NEE runs before that vertex's own roulette).  With emit_nee 1 the expectation is expected() + nee_reach() * s_d, s_d its balance-heuristic share."""
    T, S = loop(rho, max_depth)
    return S[max_depth - 1] * T[max_depth - 1] * _c3(rho) * _c3(Le)


def l_inf(Le, rho):
    return _c3(Le) / (1.0 - _c3(rho))


def variance_bound(Le, rho, max_depth, nee, mu):
    """Upper bound on the variance of one sample in the EMPTY room, per channel; derived, not measured.  Let M be the number of shaded vertices: M >= min(5, d),
    P(M >= m) = S[m - 1] from loop().  emit_nee 0: the sample IS B(M) = Le sum_(k<M) T_k.  emit_nee 1: vertex k adds its BSDF hit, w T_k Le with w <= 1, and its NEE
    sample T_k Le f cos / (p_light + p_bsdf) <= T_k Le f cos / p_bsdf = rho T_k Le (balance heuristic, whatever 1 / numPick sits in p_light): the sample is at most
    B(M) = (1 + rho) Le sum_(k<M) T_k, increasing in M.  M depends on the roulette's draws alone (T_k is the same for every path), not on where the path went,
    so given M = m the sample has the mean of a room walked m vertices deep: U(m) = Le (sum_(k<m) T_k + s rho T_(m-1)) with the last vertex's share s <= 1 (0 without
    NEE).  0 <= X <= B(m) gives X^2 <= B(m) X (Bhatia-Davis, per survival class):  V = E[X^2] - mu^2 <= sum_m P(M = m) B(m) U(m) - mu^2; without NEE, B = U = X."""
    Le, rho = _c3(Le), _c3(rho)
    T, S = loop(rho, max_depth)
    run = np.cumsum(T[:max_depth] * Le, axis=0)  # run[m - 1] = Le sum_(k<m) T_k
    B = run * ((1.0 + rho) if nee else 1.0)
    Um = run + (T[:max_depth] * rho * Le if nee else 0.0)
    pm = S[:max_depth] - np.append(S[1:max_depth], 0.0)  # P(M = m), m = 1 .. d
    assert abs(pm.sum() - 1) < 1e-12 and (pm >= 0).all()
    return (pm[:, None] * B * Um).sum(0) - _c3(mu) ** 2


def variance_bound_objects(Le, rho, nee, mu_lo):
    """The same for a room with white lossless objects in it (gray rho), where vertices are walls or objects in an order the geometry decides.  Objects leave T
    alone, so behind vertex 4 -- the first roulette -- T = rho^j, j in 0 .. 5 the walls among vertices 0 .. 4, which have added at most c Le sum_(i<j) rho^i,
    c = 1 + rho with NEE, 1 without.  The path survives that roulette with p = rho^j; a survivor has T <= 1 from then on, every later wall vertex adds at most c Le
    and is survived with p = max T <= rho: the walls behind vertex 4 number at most 1 + G, P(G >= i) = rho^i.  B_j = c Le (sum_(i<j) rho^i + Bern(rho^j) (1 + G)),
    E(1 + G) = 1 / (1 - rho), E(1 + G)^2 = (1 + rho) / (1 - rho)^2; the bound is max_j E[B_j^2] - mu_lo^2 with mu_lo a lower bound on the mean (0 is one)."""
    Le, rho = _c3(Le), _c3(rho)
    assert (rho == rho[0]).all() and no_cut_condition(rho)
    r = rho[0]
    c = (1.0 + r) if nee else 1.0
    e1, e2 = 1.0 / (1.0 - r), (1.0 + r) / (1.0 - r) ** 2
    worst = 0.0
    for j in range(6):
        a, q = sum(r ** i for i in range(j)), r ** j
        worst = max(worst, a * a + 2 * a * q * e1 + q * e2)
    return (c * Le) ** 2 * worst - _c3(mu_lo) ** 2


def camera_rays(view_to_world, clip_to_view, n, rng):
    """generate_camera_ray in float64 for image-plane points uniform over the whole image (= a uniform pixel with a uniform jitter): origin, (n, 3) unit directions"""
    V, C = np.asarray(view_to_world, np.float64).reshape(4, 4), np.asarray(clip_to_view, np.float64).reshape(4, 4)
    ndc = np.concatenate([rng.random((n, 2)) * 2 - 1, np.ones((n, 2))], 1)
    vs = ndc @ C.T
    vs[:, 3] = 0.0
    d = (vs @ V.T)[:, :3]
    return V[:3, 3].copy(), d / np.linalg.norm(d, axis=1, keepdims=True)


def walk(Le, rho, max_depth, origin, dirs, rng, nee=False, num_pick=1, half=1.0):
    """n paths through the box [-half, half]^3 in float64, the loop above restated with (nee) DESIGN.md's emitter NEE: a wall point uniform by area (every wall has
    the same Le, so luminance / sum w = 1 / area), emit_pdf = dist^2 / (cos_e area), the pick's 1 / num_pick in both techniques' p_light (the other num_pick - 1
    entries of the pick light nothing), balance heuristic.  -> per-path radiance L, the last shaded vertex's NEE term, the number of shaded vertices M."""
    Le, rho = _c3(Le), _c3(rho)
    d = np.asarray(dirs, np.float64)
    n, rows, area = len(d), np.arange(len(d)), 24.0 * half * half
    o = np.array(np.broadcast_to(np.asarray(origin, np.float64), (n, 3)))
    T, L, alive = np.ones((n, 3)), np.zeros((n, 3)), np.ones(n, bool)
    last_pdf, last_nee, M, cuts = np.zeros(n), np.zeros((n, 3)), np.zeros(n, np.int64), 0
    for k in range(max_depth):
        nz = d != 0
        tt = np.where(nz, (np.sign(d) * half - o) / np.where(nz, d, 1.0), np.inf)  # the slabs: the exit of a ray that starts inside
        ax = tt.argmin(1)
        t, sg = tt[rows, ax], np.sign(d[rows, ax])
        x = o + t[:, None] * d
        x[rows, ax] = sg * half
        nrm = np.zeros((n, 3))
        nrm[rows, ax] = -sg  # inwards
        w = np.ones(n)
        if nee and k > 0:  # an emitter hit at depth > 0 (no bounce here is specular)
            p_l = t * t / (np.abs(d[rows, ax]) * area) / num_pick
            w = last_pdf / (last_pdf + p_l)
        L += alive[:, None] * T * Le * w[:, None]
        M += alive
        if nee:
            pick = rng.random(n) < 1.0 / num_pick
            face = rng.integers(0, 6, n)
            fa, fs = face // 2, (face % 2) * 2.0 - 1.0
            y = (rng.random((n, 3)) * 2 - 1) * half
            y[rows, fa] = fs * half
            v = y - x
            dist = np.linalg.norm(v, axis=1)
            cs, ce = (nrm * v).sum(1) / dist, fs * v[rows, fa] / dist  # n_y = -fs e_fa: cos_e = -n_y . L
            ok = pick & alive & (cs > 0) & (ce > 0)
            p_l, p_b = dist * dist / (np.where(ok, ce, 1.0) * area) / num_pick, cs / np.pi
            c = T * rho * Le * np.where(ok, (cs / np.pi) / (p_l + p_b), 0.0)[:, None]  # T Le / p_l * p_l / (p_l + p_b) * rho cos / pi
            L += c
            if k == max_depth - 1:
                last_nee = c
        u1, phi = rng.random(n), 2 * np.pi * rng.random(n)  # cosine_hemisphere about the wall's normal (u1 < 1: cosT > 0, the absorb branch has measure zero)
        r, cz = np.sqrt(u1), np.sqrt(1 - u1)
        nd = np.zeros((n, 3))
        nd[rows, (ax + 1) % 3], nd[rows, (ax + 2) % 3], nd[rows, ax] = r * np.cos(phi), r * np.sin(phi), -sg * cz
        o, d, last_pdf = x, nd, cz / np.pi
        T = T * rho
        if k >= RR_FROM:
            p = T.max(1)
            alive = alive & ~(rng.random(n) > p)
            T = T * (1.0 / (p + RR_EPS))[:, None]
        cut = (T * T).sum(1) < CUT
        cuts += int((cut & alive).sum())
        alive = alive & ~cut
    return {"L": L, "last_nee": last_nee, "M": M, "cuts": cuts}


def last_vertex_share(Le, rho, max_depth, origin, dirs, rng, num_pick=1):
    """s_d and its standard error: the last shaded vertex's NEE term over nee_reach(), per path (paths dead by then count 0 on both sides of the quotient)"""
    r = walk(Le, rho, max_depth, origin, dirs, rng, nee=True, num_pick=num_pick)
    reach = nee_reach(Le, rho, max_depth)
    c = int(np.argmax(reach))
    q = r["last_nee"][:, c] / reach[c]
    return float(q.mean()), float(q.std(ddof=1) / np.sqrt(len(q))), r
