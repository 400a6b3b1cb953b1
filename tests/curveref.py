"""The round cubic B-spline curve primitive restated in numpy float64 from its definition ("Curve intersection against float64"), and the
bounds a float32 intersector is held to against it.  numpy only; nothing of the product's or the checker's intersector is read or restated here.
tests/test_curve_hairscale_cpu.py holds the CPU checker against it, tests/test_gpu_curve_hairscale.py the device.

The definition.  A segment has four control points (x, y, z, radius); its axis C(u) and radius r(u), u in [0, 1], are the uniform cubic B-spline of them
(hitref.bspline, the basis tests/test_oracle_golden.py pins).  Its swept volume is the union of the spheres (C(u), r(u)).  A ray o + t d ENTERS the volume of a set of
segments at the first t in (tmin, tmax) at which the point passes from outside every sphere to inside one.

How it is found.  For one sphere the entry is closed form: with the unit direction e = d / |d| and w = C(u) - o, the line passes the centre at distance
p(u) = sqrt(|w|^2 - (w . e)^2); it meets the sphere iff phi(u) = p(u) - r(u) <= 0, entering at s_in(u) = w . e - sqrt(r^2 - p^2) and leaving at
s_out(u) = w . e + sqrt(r^2 - p^2) (s = t |d|, a distance).  The line is inside the volume of a stretch of curve over [min_u s_in, max_u s_out] (one interval, for a
stretch the ray crosses once -- every stretch here is an eighth of a segment).  So:
  1. cull: a segment's axis lies in the hull of its control points and its radius in the hull of their radii, so the line must pass its bounding sphere;
     the axis over [k/8, (k+1)/8] lies within |C''|_max / 512 of its chord, so the line must pass the chord (closed-form closest approach of two lines, clamped) that
     near -- the bracket;
  2. refine: on each surviving eighth, minimise F(u) = s_in(u) where phi(u) <= 0, BIG + phi(u) elsewhere, by repeated 33-point grids that shrink 8 x around the best
     sample (phi leads the grid into the interval where the line meets the spheres however thin the tube is; s_in is convex there for a near-straight stretch); the same for
     -s_out;
  3. sweep the intervals of a strand's stretches in order of s_in: the ray is inside the strand while an interval that began before is still open; the first interval
     that begins after tmin |d| while none is open is the entry into that strand; the earliest over the strands is the entry.
o is moved along the line to the foot of the segment's centre first (w stays of the size of the segment: |w|^2 - (w . e)^2 does not cancel at distance 300).  The
coordinates themselves are float64: at magnitude L they are known to 1.1e-16 L, 3e-14 at L = 300 -- 2e-9 of the thinnest radius used (2e-5).

No (t x u) scan anywhere: work is proportional to the (ray, eighth) pairs that survive the cull, a handful per ray at hair scale.

tests/test_curve_hairscale_cpu.py::test_reference_agrees_with_the_dense_scan validates it against the dense scan of tests/test_oracle_intersect.py on that test's thick segment.

The u reported.  `u` is the parameter of the sphere entered first.  An intersector that works on the tangent cone reports the parameter of the FOOT of the hit point on
the axis, (P - C(u)) . C'(u) = 0 (hitref's module docstring: the offset surface); the two differ by r r' / |C'|^2 on a tapering strand.  `u_foot` is that foot, by Newton's
iteration from `u`; the tests compare with it.

Every bound below is a count of roundings, U = 2^-24 each, in the style of hitref.py; its docstring is the derivation."""
import numpy as np

from tests.hitref import U, bspline, instance_matrix, segment_control_points

BIG = 1e12
PIECES = 8  # stretches per segment
GRID = 33  # samples per refinement level; the window shrinks to 4 / 32 of itself
LEVELS = 10  # (1 / 8) * (1 / 8)^10 = 1e-10 of a segment (the minimum is quadratic: t is good to its square)


def _eval(q, u):
    """q (C, 4, 4), u (C, K) -> centre (C, K, 3), radius (C, K)"""
    c = bspline(q[:, None], u)
    return c[..., :3], c[..., 3]


def _line_chord_distance(o, e, a, b):
    """smallest distance between the line o + s e (|e| = 1; (C, 3) each) and the chord a -> b, closed form"""
    ab = b - a
    ao = a - o
    ee, ff, ef = 1.0, (ab * ab).sum(-1), (ab * e).sum(-1)
    den = ee * ff - ef * ef  # (>= 0; 0: parallel)
    # the chord's parameter of the closest approach of the two lines, clamped to the chord
    v = np.where(den > 1e-300, ((ao * e).sum(-1) * ef - (ao * ab).sum(-1) * ee) / np.where(den > 1e-300, den, 1.0), 0.0)
    v = np.clip(v, 0.0, 1.0)
    p = a + v[..., None] * ab - o
    return np.sqrt(np.maximum((p * p).sum(-1) - (p * e).sum(-1) ** 2, 0.0))


def _refine(q, o, e, lo, hi, sign):
    """minimise F over [lo, hi] per candidate: sign = +1: F = s_in where the line meets the sphere; sign = -1: F = -s_out.  -> (u, s, phi at u)"""
    lin = np.linspace(0.0, 1.0, GRID)
    lo, hi = lo.copy(), hi.copy()
    for _ in range(LEVELS):
        u = lo[:, None] + (hi - lo)[:, None] * lin[None, :]
        c, r = _eval(q, u)
        w = c - o[:, None, :]
        b = (w * e[:, None, :]).sum(-1)
        p2 = np.maximum((w * w).sum(-1) - b * b, 0.0)
        phi = np.sqrt(p2) - r
        root = np.sqrt(np.maximum(r * r - p2, 0.0))
        F = np.where(phi <= 0.0, sign * b - root, BIG + phi)
        j = np.argmin(F, axis=1)
        k = np.arange(len(j))
        best_u, best_F, best_phi = u[k, j], F[k, j], phi[k, j]
        lo, hi = u[k, np.maximum(j - 2, 0)], u[k, np.minimum(j + 2, GRID - 1)]
    return best_u, np.where(best_phi <= 0.0, sign * best_F, np.nan), best_phi


def _min_clearance(q, o, e, lo, hi):
    """min over [lo, hi] of phi(u) / r(u) per candidate, and its u"""
    lin = np.linspace(0.0, 1.0, GRID)
    lo, hi = lo.copy(), hi.copy()
    for _ in range(LEVELS):
        u = lo[:, None] + (hi - lo)[:, None] * lin[None, :]
        c, r = _eval(q, u)
        w = c - o[:, None, :]
        b = (w * e[:, None, :]).sum(-1)
        rel = (np.sqrt(np.maximum((w * w).sum(-1) - b * b, 0.0)) - r) / r
        j = np.argmin(rel, axis=1)
        k = np.arange(len(j))
        best_u, best = u[k, j], rel[k, j]
        lo, hi = u[k, np.maximum(j - 2, 0)], u[k, np.minimum(j + 2, GRID - 1)]
    return best, best_u


def foot(q, p, u):
    """the root of (p - C(u)) . C'(u) = 0 next to u, Newton's iteration: q (N, 4, 4), p (N, 3), u (N,)"""
    u = np.array(u, np.float64)
    for _ in range(20):
        c0, c1, c2 = bspline(q, u)[:, :3], bspline(q, u, 1)[:, :3], bspline(q, u, 2)[:, :3]
        g = ((p - c0) * c1).sum(-1)
        dg = -(c1 * c1).sum(-1) + ((p - c0) * c2).sum(-1)
        u = u - g / dg
    return u


def surface_distance(q, p, u0):
    """| |p - C(u*)| - r(u*) | for the foot u* of p next to u0: the distance of p from the segment's offset surface"""
    u = foot(q, p, u0)
    c = bspline(q, u)
    return np.abs(np.linalg.norm(p - c[:, :3], axis=-1) - c[:, 3])


def first_entry(o, d, segs, tmin=0.0, tmax=np.inf, matrix=None, only=None, strand=None, block=256):
    """o, d (N, 3): the rays as given (widened exactly by the caller's float64 conversion), d of any length; segs (S, 4, 4): control points (x, y, z, radius) in object space;
    matrix: the 3 x 4 object-to-world matrix of the instance (None: identity) -- the ray is taken to object space in float64, t stays the parameter of the ray as given;
    tmin, tmax: scalars or (N,); only (N,): ray i is held against segment only[i] alone; strand (S,): which strand a segment belongs to (default: each its own) --
    the segments of a strand continue one another, so passing from one into the next is no entry; passing into ANOTHER strand's tube is one even from inside a tube
    (a ray tracer's surfaces are per strand; with the origin outside every tube the two readings agree).
    -> dict of (N,) arrays:
      hit, t, seg, u, u_foot: the first entry (t nan, seg -1 on a miss);
      depth: the signed clearance of the ray's LINE (t in (tmin, inf)) from the tube surface relative to the radius there, min over all of segs of (p(u) - r(u)) / r(u)
             restricted to spheres whose closest approach lies behind tmin: < 0 the line enters the volume, > 0 it passes it; inf where the cull left nothing (clearance
             beyond every bracket: a miss by more than a radius);
      depth_seg, depth_u: where that minimum is;
      edge: the smallest |clearance| over every local minimum of the clearance along the segments the line comes near: how close the ray is to grazing ANY tube, not
            only the one it enters;
      angle: between the ray and the axis' tangent at the entry (at depth_u for a miss), radians in [0, pi / 2];
      radius, speed, bend: r, |C'|, |C''| at the entry (at depth_u for a miss);
      distance: t |d| at the entry (the distance to the closest approach for a miss);
      origin_inside: the point at tmin lies inside the volume;
      cps (N, 4, 4): the control points of that segment; o_obj, d_obj: the ray in object space."""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    tmin = np.broadcast_to(np.asarray(tmin, np.float64), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, np.float64), (n,))
    segs = np.asarray(segs, np.float64)
    strand = np.arange(len(segs)) if strand is None else np.asarray(strand)
    if matrix is not None:
        Mx = np.asarray(matrix, np.float64).reshape(3, 4)
        Mi = np.linalg.inv(Mx[:, :3])
        o, d = (o - Mx[:, 3]) @ Mi.T, d @ Mi.T
    dl = np.linalg.norm(d, axis=1)
    e = d / dl[:, None]
    P3, R = segs[..., :3], segs[..., 3]
    centre = P3.mean(axis=1)
    bound = np.linalg.norm(P3 - centre[:, None, :], axis=2).max(axis=1) + R.max(axis=1)
    sag = np.maximum(np.linalg.norm(P3[:, 0] - 2 * P3[:, 1] + P3[:, 2], axis=1), np.linalg.norm(P3[:, 1] - 2 * P3[:, 2] + P3[:, 3], axis=1)) / (8.0 * PIECES * PIECES)
    knots = np.linspace(0.0, 1.0, PIECES + 1)
    ends = bspline(segs[:, None], knots[None, :])[..., :3]  # (S, PIECES + 1, 3)
    out = {"hit": np.zeros(n, bool), "t": np.full(n, np.nan), "seg": np.full(n, -1), "u": np.full(n, np.nan), "u_foot": np.full(n, np.nan),
           "depth": np.full(n, np.inf), "edge": np.full(n, np.inf), "depth_seg": np.full(n, -1), "depth_u": np.full(n, np.nan), "origin_inside": np.zeros(n, bool)}
    cand = []  # (ray, seg, piece) triples
    for i0 in range(0, n, block):
        sl = slice(i0, min(n, i0 + block))
        w = centre[None, :, :] - o[sl, None, :]
        b = (w * e[sl, None, :]).sum(-1)
        p2 = (w * w).sum(-1) - b * b
        # (|w|^2 - b^2 cancels at a large distance: 4e-16 |w|^2 of slack keeps the cull conservative)
        near = p2 <= (3.0 * bound[None, :]) ** 2 + 1e-14 * (w * w).sum(-1)
        if only is not None:
            near &= np.arange(len(segs))[None, :] == np.asarray(only)[sl, None]
        ri, si = np.nonzero(near)
        if not len(ri):
            continue
        ri = ri + i0
        rr, ss, kk = np.repeat(ri, PIECES), np.repeat(si, PIECES), np.tile(np.arange(PIECES), len(ri))
        # the line, re-based at the foot of the segment's centre
        ob = o[rr] + ((centre[ss] - o[rr]) * e[rr]).sum(-1)[:, None] * e[rr]
        dist = _line_chord_distance(ob, e[rr], ends[ss, kk], ends[ss, kk + 1])
        keep = dist <= 3.0 * R[ss].max(axis=1) + sag[ss]  # (3 radii: the clearance of near misses is wanted too)
        cand.append(np.stack([rr[keep], ss[keep], kk[keep]], 1))
    if not cand or not sum(len(c) for c in cand):
        return _finish(out, o, d, dl, e, segs, tmin)
    cand = np.concatenate(cand)
    rr, ss, kk = cand[:, 0], cand[:, 1], cand[:, 2]
    base = ((centre[ss] - o[rr]) * e[rr]).sum(-1)
    ob = o[rr] + base[:, None] * e[rr]
    q = segs[ss]
    lo, hi = knots[kk], knots[kk + 1]
    u_in, s_in, _ = _refine(q, ob, e[rr], lo, hi, +1.0)
    _, s_out, _ = _refine(q, ob, e[rr], lo, hi, -1.0)
    s_in, s_out = s_in + base, s_out + base
    clr, clr_u = _min_clearance(q, ob, e[rr], lo, hi)
    # the clearance counts where the closest approach lies in front of tmin
    c_at, _ = _eval(q, clr_u[:, None])
    s_at = ((c_at[:, 0] - o[rr]) * e[rr]).sum(-1)
    clr = np.where(s_at > tmin[rr] * dl[rr], clr, np.inf)
    order = np.lexsort((np.where(np.isnan(s_in), np.inf, s_in), rr))
    rr_o = rr[order]
    starts = np.searchsorted(rr_o, np.arange(n), "left")
    stops = np.searchsorted(rr_o, np.arange(n), "right")
    for i in np.nonzero(stops > starts)[0]:
        idx = order[starts[i]:stops[i]]
        j = np.argmin(clr[idx])
        # (a minimum at the end of a stretch is not a minimum of the tube's clearance: the next stretch continues it)
        inner = (clr_u[idx] > lo[idx] + 1e-9) & (clr_u[idx] < hi[idx] - 1e-9)
        if inner.any():
            out["edge"][i] = np.abs(clr[idx][inner]).min()
        if clr[idx][j] < out["depth"][i]:
            out["depth"][i], out["depth_seg"][i], out["depth_u"][i] = clr[idx][j], ss[idx][j], clr_u[idx][j]
        smin, smax = tmin[i] * dl[i], tmax[i] * dl[i]
        ok = ~np.isnan(s_in[idx])
        best_s = np.inf
        for st in np.unique(strand[ss[idx][ok]]):  # (a strand at a time: its stretches continue one another, another strand's tube is another surface)
            mine = idx[ok & (strand[ss[idx]] == st)]  # (in order of s_in)
            before = s_in[mine] <= smin
            open_until = s_out[mine][before].max() if before.any() else -np.inf
            out["origin_inside"][i] |= open_until > smin
            for c in mine[~before]:
                if s_in[c] <= open_until:
                    open_until = max(open_until, s_out[c])
                    continue
                if s_in[c] < smax and s_in[c] < best_s:
                    best_s = s_in[c]
                    out["hit"][i], out["t"][i], out["seg"][i], out["u"][i] = True, s_in[c] / dl[i], ss[c], u_in[c]
                break
    return _finish(out, o, d, dl, e, segs, tmin)


def _finish(out, o, d, dl, e, segs, tmin):
    n = len(o)
    hit = out["hit"]
    seg = np.where(hit, out["seg"], out["depth_seg"])
    u = np.where(hit, out["u"], out["depth_u"])
    have = seg >= 0
    for key in ("angle", "radius", "speed", "bend", "distance"):
        out[key] = np.full(n, np.nan)
    if have.any():
        q = segs[seg[have]]
        uu = u[have]
        c0, c1, c2 = bspline(q, uu), bspline(q, uu, 1), bspline(q, uu, 2)
        sp = np.linalg.norm(c1[:, :3], axis=1)
        cosang = np.abs((c1[:, :3] * e[have]).sum(-1)) / sp
        out["angle"][have] = np.arccos(np.clip(cosang, 0.0, 1.0))
        out["radius"][have], out["speed"][have], out["bend"][have] = c0[:, 3], sp, np.linalg.norm(c2[:, :3], axis=1)
        out["distance"][have] = np.where(hit[have], out["t"][have] * dl[have], ((c0[:, :3] - o[have]) * e[have]).sum(-1))
        if hit.any():
            p = o[hit] + out["t"][hit][:, None] * d[hit]
            out["u_foot"][hit] = foot(segs[out["seg"][hit]], p, out["u"][hit])
    out["o_obj"], out["d_obj"] = o, d
    out["cps"] = segs[np.maximum(seg, 0)] if len(segs) else np.zeros((n, 4, 4))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def curve_instances(arr):
    """[(instance id, 3 x 4 matrix, control points (S, 4, 4), strand of each segment (S,))] of the curve instances (type 2) of the flat scene arrays"""
    res = []
    for i, rec in enumerate(arr["instances"]):
        if int(rec["type"]) != 2:
            continue
        cu = arr["curves"][int(rec["geom_id"])]
        counts = arr["curve_vertex_counts"][int(cu["vertex_counts_start"]):int(cu["vertex_counts_start"]) + int(cu["vertex_counts_count"])]
        nseg = int(sum(max(int(c) - 3, 0) for c in counts))
        strand = np.concatenate([np.full(max(int(c) - 3, 0), k) for k, c in enumerate(counts)]) if nseg else np.zeros(0, int)
        res.append((i, instance_matrix(arr, i), segment_control_points(arr, i, np.arange(nseg)), strand))
    return res


def trace(arr, rays):
    """first_entry over every curve instance of a scene; rays: records with origin, tmin, dir, tmax.  The entry into the union of the instances' volumes is the
    smallest of their entries (the instances of these tests do not overlap).  Adds `inst` (-1: miss), `kappa` (ratio of M3's extreme singular values) and `world_scale` =
    |origin - translation| times |inverse(M3)|, the magnitude the object-space origin is made from (0 under the bit-exact identity: x * 1 + y * 0 + z * 0 rounds nothing)."""
    o, d = np.asarray(rays["origin"], np.float64), np.asarray(rays["dir"], np.float64)
    tmin, tmax = np.asarray(rays["tmin"], np.float64), np.asarray(rays["tmax"], np.float64)
    best = None
    for inst, Mx, segs, strand in curve_instances(arr):
        r = first_entry(o, d, segs, tmin, tmax, Mx, strand=strand)
        r["inst"] = np.where(r["hit"], inst, -1)
        sv = np.linalg.svd(Mx[:, :3], compute_uv=False)
        r["world_scale"] = np.zeros(len(o)) if np.array_equal(Mx, np.eye(4)[:3]) else np.abs(o - Mx[:, 3]).max(axis=1) / sv[-1]
        r["kappa"] = np.full(len(o), sv[0] / sv[-1])
        if best is None:
            best = r
            continue
        # the nearer entry wins; among misses the smaller clearance describes the ray
        take = (r["hit"] & (~best["hit"] | (r["t"] < best["t"]))) | (~r["hit"] & ~best["hit"] & (r["depth"] < best["depth"]))
        inside, edge = best["origin_inside"] | r["origin_inside"], np.minimum(best["edge"], r["edge"])
        for k in best:
            best[k] = np.where(take.reshape((-1,) + (1,) * (best[k].ndim - 1)), r[k], best[k])
        best["origin_inside"], best["edge"] = inside, edge
    return best


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
CURVE_DU = 5e-5  # the intersector ends its iteration when a step in u is shorter than this
ON_TUBE = 1.001  # ... and accepts the point if its squared radial distance is within this factor of the cone's squared radius: 5e-4 in the distance
K_LAT = 20.0
K_Z = 29.0
K_POLY = 13.0
K_CONE = 16.0
K_XFORM = 12.0
M_CAP = 0.5


def lateral_error(distance, length, world_scale=0.0, kappa=1.0):
    """How far (a length) an fp32 intersector that works in ray-centric coordinates may misplace the axis relative to the ray, across the ray.
    The control points q are taken to the frame (bx, by, e) of the unit direction e as ((q - o) . bx, (q - o) . by, (q - o) . e); |q - o| <= `distance` = D.
      q - o: one rounding per component, U D;
      e = d (1 / |d|): the reciprocal length's error only scales; the product rounds once per component: e is off the true direction by U, U D across at the curve;
      bx, by from e (a branch-free orthonormal basis: a quotient, a sum, two products and a sum per component, 4 U each, |dbx| <= 4 sqrt 3 U = 7 U): what counts is
        that bx stays perpendicular to e: 7 U D;
      the dot product: three products and two sums on terms <= D |bx_i|: 5 U D;
    14 U D per axis, sqrt 2 for the two: K_LAT = 20.  The polynomial coefficients from the four transformed points and Horner's rule (hitref.curve_normal_bound: 7 + 6
    roundings) act on the ACROSS coordinates, which are of the size of the segment, `length`: K_POLY U length.  Under an instance transform the object-space origin is
    inverse(M3) (o - T) in fp32: the difference rounds relative to ITSELF, U |o - T| however far from zero o and T lie (an implementation that folded the translation into the
    inverse, inverse(M3) o - inverse(M3) T, would round at |T| instead and miss this bound under a far translation); the 3 x 3 product with once-rounded entries, 6 U;
    the direction likewise, 5 U of a unit vector shown at distance D: K_XFORM = 12 on max(world_scale, D), world_scale = |o - T| |inverse(M3)|, amplified by kappa when the space is sheared (the radius is object
    space's, the error the product's in any direction)."""
    return K_LAT * U * distance + K_POLY * U * length + K_XFORM * U * np.maximum(world_scale, distance) * kappa * (np.asarray(world_scale) > 0)


def margin(distance, radius, speed, length, world_scale=0.0, kappa=1.0):
    """m: a ray whose line passes the axis at rho r is decided by float64 if rho <= 1 - m (hit) or rho >= 1 + m (miss):
      lateral_error / r: the axis misplaced across the ray;
      K_CONE U: the tangent cone's quadratic (some 16 operations on quantities relative to r |C'|: no distance in it);
      ON_TUBE: points up to 1.0005 r from the axis are accepted: 5e-4;
      CURVE_DU |C'| / r: the iteration stops within CURVE_DU of the parameter it would converge to, CURVE_DU |C'| along the axis, and decides on the tangent cone there;
        counted in full against the radius (the cone differs from the surface only in second order; this is the conservative reading)."""
    return lateral_error(distance, length, world_scale, kappa) / radius + K_CONE * U + (np.sqrt(ON_TUBE) - 1.0) + CURVE_DU * speed / radius


def grazing(angle, rho, m):
    """1 / (sin(angle to the tangent) sqrt(1 - rho^2)): a displacement across the ray moves the entry along the ray by this factor; rho taken m nearer to 1
    (the intersector's own rho may be that much larger)"""
    rho = np.minimum(np.abs(rho) + m, 1.0 - 1e-3)
    return 1.0 / (np.sin(angle) * np.sqrt(1.0 - rho * rho))


def t_bar(distance, radius, speed, bend, length, angle, rho, world_scale=0.0, kappa=1.0):
    """|t - t_ref| |d| <= this, a length.  Along the ray: the z coordinate of the curve point, (q - o) . e, carries the subtraction (1), e's scale (|d| is off by the
    root's and the reciprocal's roundings and the sum of squares': 4), the dot product (5), the polynomial (13, on a coordinate of size D here), the sum s + z and the
    product with 1 / |d| (2), the transform of the ray's origin along the ray (3), and t rounds to fp32 (1): K_Z = 29 on D.  Across the ray: lateral_error and the
    cone's own K_CONE U r, times grazing().  The cone the hit lies on is tangent at a parameter within CURVE_DU of the entry's: CURVE_DU^2 |C''| / 2 off the surface,
    times grazing()."""
    m = margin(distance, radius, speed, length, world_scale, kappa)
    g = grazing(angle, rho, m)
    return K_Z * U * np.maximum(distance, world_scale * (np.asarray(world_scale) > 0)) + (lateral_error(distance, length, world_scale, kappa) + K_CONE * U * radius + 0.5 * CURVE_DU ** 2 * bend) * g


def u_bar(distance, radius, speed, bend, length, angle, rho, world_scale=0.0, kappa=1.0):
    """|u - u_foot| <= this: CURVE_DU, and the hit point's displacement -- t_bar along the ray and lateral_error across -- shown along the axis, / |C'|, / (1 - r |C''| / |C'|^2)
    on the inside of a bend"""
    move = t_bar(distance, radius, speed, bend, length, angle, rho, world_scale, kappa) + lateral_error(distance, length, world_scale, kappa)
    return CURVE_DU + move / speed / np.maximum(1.0 - radius * bend / speed ** 2, 0.5)


def surf_bar(distance, radius, speed, bend, length, taper, world_scale=0.0, kappa=1.0):
    """the reported point o + t d (float64 of the fp32 t) lies within this times r of the tube surface.  t's error counts only by its component along the surface
    normal, which is what grazing() divided by: the factor cancels.  K_Z U D along the ray (shown on the normal: <= 1) + lateral_error + K_CONE U r + the cone's
    second-order CURVE_DU^2 |C''| / 2; and the surface found is the offset surface, which the envelope of the spheres lies r a^2 / 2 inside of, a = r' / |C'| = `taper`
    (hitref's module docstring).  Relative to r."""
    return (K_Z * U * np.maximum(distance, world_scale * (np.asarray(world_scale) > 0)) + lateral_error(distance, length, world_scale, kappa) + 0.5 * CURVE_DU ** 2 * bend) / radius + K_CONE * U + 0.5 * taper ** 2


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the decided set and the comparison
# ---------------------------------------------------------------------------------------------------------------------------------------------
MIN_ANGLE = np.radians(20.0)
U_LO, U_HI = 0.03, 0.97


def judge(ref, got_hit, got_t, got_u, dlen, world_scale=0.0, kappa=1.0, allow_inside=False):
    """ref: first_entry's / trace's result; got_*: the intersector's answer per ray (hit, t, u); dlen = |d| of the ray as given.
    The decided set: the origin outside every tube (allow_inside: or anywhere -- a ray whose tmin was put inside a tube on purpose); the margin m(ray) <= M_CAP; every tube the line comes near cleared or entered by more than m (`edge`); a hit
    enters at u in [0.03, 0.97] at >= 20 degrees to the tangent.
    -> dict: decided, m, agree (decision equal; meaningful on decided rays), and for decided hits both sides report, as multiples of their bars: rt, ru, rs (nan elsewhere)."""
    n = len(ref["hit"])
    seg = np.where(ref["hit"], ref["seg"], ref["depth_seg"])
    have = seg >= 0
    m = np.zeros(n)
    length, taper = np.zeros(n), np.zeros(n)
    if have.any():
        q = ref["cps"][have]
        length[have] = np.linalg.norm(q[:, :, :3] - q[:, :, :3].mean(axis=1, keepdims=True), axis=2).max(axis=1)
        uu = np.where(ref["hit"], ref["u"], ref["depth_u"])[have]
        taper[have] = np.abs(bspline(q, uu, 1)[:, 3]) / ref["speed"][have]
    ws = np.broadcast_to(np.asarray(world_scale, np.float64), (n,))
    kp = np.broadcast_to(np.asarray(kappa, np.float64), (n,))
    with np.errstate(invalid="ignore"):
        m[have] = margin(np.abs(ref["distance"][have]), ref["radius"][have], ref["speed"][have], length[have], ws[have], kp[have])
        decided = (allow_inside | ~ref["origin_inside"]) & (m <= M_CAP) & (ref["edge"] >= m)
        decided &= np.where(ref["hit"], (ref["u"] >= U_LO) & (ref["u"] <= U_HI) & (ref["angle"] >= MIN_ANGLE) & (ref["depth"] <= -m), ~have | (ref["depth"] >= m))
    got_hit = np.asarray(got_hit, bool)
    out = {"decided": decided, "m": m, "agree": got_hit == ref["hit"], "rt": np.full(n, np.nan), "ru": np.full(n, np.nan), "rs": np.full(n, np.nan)}
    k = decided & ref["hit"] & got_hit
    if k.any():
        a = dict(distance=ref["distance"][k], radius=ref["radius"][k], speed=ref["speed"][k], bend=ref["bend"][k], length=length[k], world_scale=ws[k], kappa=kp[k])
        rho = 1.0 + ref["depth"][k]
        out["rt"][k] = np.abs(np.asarray(got_t, np.float64)[k] - ref["t"][k]) * np.asarray(dlen, np.float64)[k] / t_bar(angle=ref["angle"][k], rho=rho, **a)
        out["ru"][k] = np.abs(np.asarray(got_u, np.float64)[k] - ref["u_foot"][k]) / u_bar(angle=ref["angle"][k], rho=rho, **a)
        p = ref["o_obj"][k] + np.asarray(got_t, np.float64)[k][:, None] * ref["d_obj"][k]
        out["rs"][k] = surface_distance(ref["cps"][k], p, np.asarray(got_u, np.float64)[k]) / ref["radius"][k] / surf_bar(taper=taper[k], **a)
    return out


def record(key, value):
    """the measured figures of a test (quoted in DESIGN.md) -> curve_hairscale.json under `key`, in the directory the environment variable SKH_MEASURED_DIR names;
    without it they are only printed"""
    import json
    import os

    d = os.environ.get("SKH_MEASURED_DIR")
    if not d:
        return
    try:
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "curve_hairscale.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[key] = value
        json.dump(doc, open(path, "w"), indent=1)
    except (OSError, ValueError):
        pass
