"""Hit reconstruction restated in numpy float64 ("Hit reconstruction"): the camera rays the renderers
trace, the closest hit by brute force, and the surface state the reference's closest-hit program defines at it -- position, shading normal, geometric
normal, tangent frame, mapped normal, and the normal of a curve's surface from the surface's definition.  numpy only; of the product it reads the flat
scene arrays (Scene.arrays()) and nothing else; the rays and their jitter come from the checker's exports of the camera and the sampler, which are pinned elsewhere.  tests/test_hit_cpu.py holds the CPU checker against it, tests/test_gpu_hit.py the device.

Where the reference's behaviour is the definition and not the textbook's, the reference is restated (src/render/optix/OptixRender_radiance_closest_hit.cu):
  * :236-244  unpackNormal masks z with 0xfff00000 -- 12 bits, not 10 -- and divides by the float 511.99999f, which IS 512.0f: every unpacked
              component is q / 256 - 1, exact in fp32.  A vertex normal is therefore never quite of unit length, and is not renormalised before the blend.
  * :199-205  the blend is attr1 (1 - u - v) + attr2 u + attr3 v: the hit's u belongs to the triangle's SECOND vertex, v to its third.
  * :400      the shading normal goes through the normal transform, inverse(M3)^T (optixTransformNormalFromObjectToWorldSpace), and is normalised after.
  * :401-402  the geometric normal is cross(p1 - p0, p2 - p0) of the OBJECT-space vertices through the same normal transform -- not the winding of the
              world-space triangle: under a mirroring instance (det M3 < 0) it points to the other side of the world-space winding.
  * :403-404  the tangent goes through the NORMAL transform too (a tangent is a direction of the surface and would textbook-wise go through M3).
  * :405-406  the normals flip only for `inside`, which is path state (false at depth 0): a surface seen from behind keeps its normal.
  * :408      the binormal is cross(normal, tangent) in this order, from the world-space vectors; nothing is re-orthogonalised.
  * :434-436  a curve's hit point is ray origin + t direction taken to object space; its normal is the surface's through that point.
  * cuda/curve.h:320-338  a curve's surface is the OFFSET surface x = c(u) + r(u) e with e a unit vector perpendicular to c'(u) -- the sweep of a disc that stays
              perpendicular to the axis --, not the envelope of the spheres |x - c(u)| = r(u).  The two agree where r' = 0; on a strand that tapers with
              a = r' / |c'| the envelope lies r a^2 / 2 inside the offset surface (1.1e-4 r at a = 0.0146, the tapering strand of tests/test_hit_cpu.py: the
              hits of the intersector, which finds the offset surface, miss the envelope by that much) and its normal leans by asin a where the offset surface's
              leans by atan a.
The mapped normal is normalize(tangent_u x + tangent_v y + normal z) with (x, y, z) = 2 texel - 1 (base::tangent_space_normal_texture, factor 1).

U = 2^-24 is half an ulp, relative.  Every bound below is a count of roundings; its docstring is the derivation."""
import numpy as np

U = 2.0 ** -24
EDGE = 1e-4  # a hit is judged only where its smallest barycentric is further than this from 0, and the next surface further than this (relative) in t
C_ISECT = 8.0  # roundings of an fp32 ray / triangle test between its inputs and the point it finds (two edge differences, a cross product, a dot product, the quotient)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------------------------------
def sampler_jitter(w, h, sample_index, spp_total=64, seed=52):
    """the sampler's values for DIM_PIXEL_X = 0 / DIM_PIXEL_Y = 1 at depth 0 for every pixel: (h, w, 2) float32, from the checker's export of the sampler,
    which tests/test_oracle_golden.py::test_sampler_bit_exact pins bit for bit to the reference's RandomSampler.h"""
    import ctypes as C

    from tests import orklib

    ork = orklib.load()
    ys, xs = np.mgrid[0:h, 0:w]
    x, y = np.ascontiguousarray(xs.reshape(-1), np.uint32), np.ascontiguousarray(ys.reshape(-1), np.uint32)
    si, depth = np.full(w * h, sample_index, np.uint32), np.zeros(w * h, np.uint32)
    out = np.zeros((w * h, 2), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for dim in (0, 1):
        o = np.zeros(w * h, np.float32)
        ork.ork_sampler_values(p(x), p(y), p(si), spp_total, p(depth), p(np.full(w * h, dim, np.uint32)), w * h, seed, p(o))
        out[:, dim] = o
    return out.reshape(h, w, 2)


def camera_rays(params, w, h, sample_index, jitter):
    """-> (origin, direction), each (h, w, 3) float32: the ray of sample `sample_index` of every pixel, jittered by jitter[py, px] (the caller's, from the
    sampler: sampler_jitter above or the device's unit probe).  The ray is the checker's ork_camera_ray, which
    tests/test_oracle_golden.py::test_camera_ray_matches_the_reference_formula_in_fp64 holds to the float64 formula."""
    import ctypes as C

    from tests import orklib

    ork = orklib.load()
    c2v = np.ascontiguousarray(params["clip_to_view"], np.float32).reshape(16)
    v2w = np.ascontiguousarray(params["view_to_world"], np.float32).reshape(16)
    jitter = np.asarray(jitter, np.float32)
    assert jitter.shape == (h, w, 2) and int(params["subframe_index"]) == sample_index
    o, d = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    oo, dd = np.zeros(3, np.float32), np.zeros(3, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for py in range(h):
        for px in range(w):
            ork.ork_camera_ray(px, py, w, h, p(c2v), p(v2w), float(jitter[py, px, 0]), float(jitter[py, px, 1]), p(oo), p(dd))
            o[py, px], d[py, px] = oo, dd
    return o, d


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the scene arrays
# ---------------------------------------------------------------------------------------------------------------------------------------------
def instance_matrix(arr, inst):
    """the float32 3 x 4 object-to-world matrix of an instance, widened exactly"""
    return np.asarray(arr["instances"]["transform"][inst], np.float64).reshape(3, 4)


def unpack_normal(val):
    """closest_hit.cu:236-244 in float64: x = bits 0-9, y = bits 10-19, z = bits 20-31 (the 12-bit mask); the divisor is the float nearest to 511.99999"""
    val = np.asarray(val, np.uint32)
    k = float(np.float32(511.99999))
    z = ((val & np.uint32(0xFFF00000)) >> np.uint32(20)).astype(np.float64) / k * 2.0 - 1.0
    y = ((val & np.uint32(0x000FFC00)) >> np.uint32(10)).astype(np.float64) / k * 2.0 - 1.0
    x = (val & np.uint32(0x000003FF)).astype(np.float64) / k * 2.0 - 1.0
    return np.stack([x, y, z], -1)


def triangle_table(arr):
    """every triangle of every MESH instance (type 0): instance, primitive, the three global vertex indices, the instance matrix"""
    inst, prim, vid = [], [], []
    for i, rec in enumerate(arr["instances"]):
        if int(rec["type"]) != 0:
            continue
        me = arr["meshes"][int(rec["geom_id"])]
        idx = arr["indices"][int(me["index_offset"]):int(me["index_offset"]) + int(me["index_count"])].astype(np.int64).reshape(-1, 3)
        inst.append(np.full(len(idx), i)), prim.append(np.arange(len(idx))), vid.append(idx + int(me["vertex_offset"]))
    inst, prim, vid = np.concatenate(inst), np.concatenate(prim), np.concatenate(vid)
    M = np.stack([instance_matrix(arr, i) for i in inst])
    return inst, prim, vid, M


# ---------------------------------------------------------------------------------------------------------------------------------------------
# closest hit, brute force
# ---------------------------------------------------------------------------------------------------------------------------------------------
def first_hits(arr, rays):
    """rays: (origin, direction), (..., 3) float32 each, widened exactly.  Closest hit in float64 over all triangles of all mesh instances, the vertices taken
    to world space with the float32 instance matrix widened to float64.  -> dict of flat arrays over the rays:
      inst, prim   (-1: no hit);   t;   bary (N, 2): the weights of the triangle's second and third vertex;   min_bary: the smallest of the three weights;
      t_next: the second-closest hit's t (inf: none);   cos: |direction . unit world-winding normal| of the hit triangle;
      unclear: the hit -- or the miss -- hangs on less than EDGE: some triangle in front of the origin has its smallest weight within EDGE of 0, or the two
               closest hits lie within EDGE of each other in t, relatively."""
    o = np.asarray(rays[0], np.float64).reshape(-1, 3)
    d = np.asarray(rays[1], np.float64).reshape(-1, 3)
    inst, prim, vid, M = triangle_table(arr)
    P = np.asarray(arr["vertices"]["pos"], np.float64)[vid]  # (T, 3, 3)
    W = np.einsum("tij,tkj->tki", M[:, :, :3], P) + M[:, None, :, 3]
    e1, e2 = W[:, 1] - W[:, 0], W[:, 2] - W[:, 0]
    n = np.cross(e1, e2)
    s = o[:, None, :] - W[None, :, 0, :]  # (N, T, 3)
    det = -(d @ n.T)  # (N, T)
    ok = det != 0
    inv = 1.0 / np.where(ok, det, 1.0)
    t = np.einsum("ntk,tk->nt", s, n) * inv
    q = np.cross(s, d[:, None, :])
    u = np.einsum("ntk,tk->nt", q, e2) * inv
    v = -np.einsum("ntk,tk->nt", q, e1) * inv
    mb = np.minimum(np.minimum(u, v), 1.0 - u - v)
    front = ok & (t > 0)
    hit = front & (mb >= 0)
    th = np.where(hit, t, np.inf)
    k = np.argmin(th, axis=1)
    r = np.arange(len(o))
    t0 = th[r, k]
    found = np.isfinite(t0)
    th2 = th.copy()
    th2[r, k] = np.inf
    t1 = th2.min(axis=1)
    with np.errstate(invalid="ignore"):
        unclear = (front & (np.abs(mb) < EDGE)).any(axis=1) | (found & np.isfinite(t1) & (t1 - t0 < EDGE * t0))
    nn = n / np.linalg.norm(n, axis=1, keepdims=True)
    return {"inst": np.where(found, inst[k], -1), "prim": np.where(found, prim[k], -1), "tri": np.where(found, k, -1), "t": np.where(found, t0, np.nan),
            "bary": np.stack([u[r, k], v[r, k]], 1), "min_bary": mb[r, k], "t_next": t1, "cos": np.abs((d * nn[k]).sum(1)), "unclear": unclear,
            "origin": o, "dir": d}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the state at a triangle hit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def triangle_state(arr, hit, texel=None):
    """the state the reference defines at the hits of first_hits (rows of rays that miss hold nan): position, normal, geom_normal, tangent_u, tangent_v, and --
    with `texel` = the normal map's constant (r, g, b) bytes -- mapped, all world space, float64; beside them what the bounds need: kappa (ratio of the
    extreme singular values of M3), the lengths of the blended object-space normal and tangent (n_len, t_len) and of the unnormalised mapped normal (m_len),
    the largest difference between two of the triangle's vertex normals / tangents (n_spread, t_spread), size_ratio = largest coordinate / smallest altitude of the
    triangle (the larger of object and world space), and scale = the largest coordinate magnitude in the position's chain (position_bound)."""
    inst, prim, vid, M = triangle_table(arr)
    ok = hit["tri"] >= 0
    k = np.where(ok, hit["tri"], 0)
    V = arr["vertices"]
    P = np.asarray(V["pos"], np.float64)[vid[k]]  # (N, 3, 3)
    N3, T3 = unpack_normal(V["normal"][vid[k]]), unpack_normal(V["tangent"][vid[k]])
    bu, bv = hit["bary"][:, 0], hit["bary"][:, 1]
    w = np.stack([1.0 - bu - bv, bu, bv], 1)[:, :, None]
    Mk = M[k]
    M3, T = Mk[:, :, :3], Mk[:, :, 3]
    NT = np.transpose(np.linalg.inv(M3), (0, 2, 1))  # inverse(M3)^T
    p_obj = (w * P).sum(1)
    n_obj, t_obj = (w * N3).sum(1), (w * T3).sum(1)
    apply = lambda A, x: np.einsum("nij,nj->ni", A, x)
    normal = _unit(apply(NT, n_obj))
    geom = _unit(apply(NT, np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])))
    tu = _unit(apply(NT, t_obj))
    tv = np.cross(normal, tu)
    pos = apply(M3, p_obj) + T
    sv = np.linalg.svd(M3, compute_uv=False)
    out = {"position": pos, "normal": normal, "geom_normal": geom, "tangent_u": tu, "tangent_v": tv, "kappa": sv[:, 0] / sv[:, -1],
           "n_len": np.linalg.norm(n_obj, axis=1), "t_len": np.linalg.norm(t_obj, axis=1)}
    spread = lambda A: np.abs(A[:, :, None, :] - A[:, None, :, :]).max(axis=(1, 2, 3))
    out["n_spread"], out["t_spread"] = spread(N3), spread(T3)
    Wv = np.einsum("nij,nkj->nki", M3, P) + T[:, None, :]

    def ratio(X):
        a, b, c = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 2] - X[:, 1]
        area2 = np.linalg.norm(np.cross(a, b), axis=1)
        longest = np.maximum(np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)), np.linalg.norm(c, axis=1))
        return area2 / longest  # the smallest altitude

    o = hit["origin"]
    Lw = np.maximum(np.abs(Wv).max(axis=(1, 2)), np.abs(o).max(axis=1))
    Lo = np.maximum(np.abs(P).max(axis=(1, 2)), np.abs(apply(np.linalg.inv(M3), o - T)).max(axis=1))
    out["size_ratio"] = np.maximum(Lw / ratio(Wv), Lo / ratio(P))
    out["scale"] = np.maximum(Lw, (np.abs(M3).sum(2) * np.abs(P).max(axis=(1, 2))[:, None] + np.abs(T)).max(axis=1))
    if texel is not None:
        ts = 2.0 * (np.asarray(texel, np.float64)[:3] / 255.0) - 1.0
        m = tu * ts[0] + tv * ts[1] + normal * ts[2]
        out["mapped"], out["m_len"], out["ts"] = _unit(m), np.linalg.norm(m, axis=1), ts
    for key, val in out.items():
        if key != "ts":
            out[key] = np.where(ok if val.ndim == 1 else ok[:, None], val, np.nan)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the state at a curve hit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def segment_control_points(arr, inst, seg):
    """the four (x, y, z, radius) control points of segment `seg` of the curve set instance `inst` refers to: a strand of n points has n - 3 segments, segment
    i of it the points i ... i + 3; the segments of a set are numbered strand after strand"""
    cu = arr["curves"][int(arr["instances"]["geom_id"][inst])]
    counts = arr["curve_vertex_counts"][int(cu["vertex_counts_start"]):int(cu["vertex_counts_start"]) + int(cu["vertex_counts_count"])].astype(np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    start = np.concatenate([f + np.arange(max(int(c) - 3, 0)) for f, c in zip(first, counts)]) + int(cu["points_start"])
    s = start[np.asarray(seg, np.int64)]
    idx = s[..., None] + np.arange(4)
    return np.concatenate([np.asarray(arr["curve_points"], np.float64)[idx], np.asarray(arr["curve_radii"], np.float64)[idx][..., None]], -1)


def bspline(q, u, order=0):
    """the uniform cubic B-spline through the control points q (..., 4, k) at u, or its first / second derivative:
    B0 = (1 - u)^3 / 6, B1 = (3 u^3 - 6 u^2 + 4) / 6, B2 = (-3 u^3 + 3 u^2 + 3 u + 1) / 6, B3 = u^3 / 6"""
    u = np.asarray(u, np.float64)
    if order == 0:
        B = [(1 - u) ** 3, 3 * u ** 3 - 6 * u ** 2 + 4, -3 * u ** 3 + 3 * u ** 2 + 3 * u + 1, u ** 3]
    elif order == 1:
        B = [-3 * (1 - u) ** 2, 9 * u ** 2 - 12 * u, -9 * u ** 2 + 6 * u + 3, 3 * u ** 2]
    else:
        B = [6 * (1 - u), 18 * u - 12, -18 * u + 6, 6 * u]
    return sum(b[..., None] * q[..., i, :] for i, b in enumerate(B)) / 6.0


def curve_state(arr, inst, seg, p_world):
    """The normal of the surface of segment `seg` (N,) of curve instance `inst` at the world-space points p_world (N, 3), from the surface's definition and not from
    curve.h's formula.  The surface (module docstring, curve.h:320-338) is x = c(u) + r(u) e, e any unit vector perpendicular to c'(u): the parameter of the
    object-space point p = inverse(M) p_world is the root u* of g(u) = (p - c(u)) . c'(u) = 0 nearest to the point -- a scan of 513 values of u over [0, 1] for the
    smallest |p - c(u)|, then Newton's iteration on g in float64 --, and p lies on the surface iff |p - c(u*)| = r(u*).  The surface is the zero set of
    F(x) = |x - c(u(x))|^2 - r(u(x))^2 with u(x) defined by g = 0; by the implicit function theorem grad u = c' / (|c'|^2 - (x - c) . c''), so
    grad F / 2 = (x - c) - r r' c' / (|c'|^2 - (x - c) . c''): the object-space normal is its direction, the world-space one normalize(inverse(M3)^T n).
    (tests/test_hit_cpu.py holds this against the cross product of the surface's finite-difference partial derivatives and against a cone's elementary normal.)
    -> dict: normal (N, 3), u (N,), residual = | |p - c(u*)| - r(u*) |, radius = r(u*), kappa, scale (curve_normal_bound's L), bend = |c''(u*)| / |c'(u*)|, speed = |c'(u*)|"""
    p_world = np.asarray(p_world, np.float64)
    Mx = instance_matrix(arr, inst)
    M3, T = Mx[:, :3], Mx[:, 3]
    Mi = np.linalg.inv(M3)
    p = (p_world - T) @ Mi.T
    q = segment_control_points(arr, inst, seg)  # (N, 4, 4)
    us = np.linspace(0.0, 1.0, 513)
    c = bspline(q[:, None], us[None, :])  # (N, 513, 4)
    u = us[np.argmin(np.linalg.norm(p[:, None, :] - c[..., :3], axis=-1), axis=1)]
    for _ in range(30):
        c0, c1, c2 = bspline(q, u), bspline(q, u, 1), bspline(q, u, 2)
        dlt = p - c0[:, :3]
        g = (dlt * c1[:, :3]).sum(1)
        dg = -(c1[:, :3] ** 2).sum(1) + (dlt * c2[:, :3]).sum(1)
        u = u - g / dg
    c0, c1, c2 = bspline(q, u), bspline(q, u, 1), bspline(q, u, 2)
    dlt = p - c0[:, :3]
    dist = np.linalg.norm(dlt, axis=1)
    n_obj = dlt - (c0[:, 3] * c1[:, 3] / ((c1[:, :3] ** 2).sum(1) - (dlt * c2[:, :3]).sum(1)))[:, None] * c1[:, :3]
    sv = np.linalg.svd(M3, compute_uv=False)
    scale = max(float(np.abs(p_world).max()), float(np.abs(T).max())) * float(1.0 / sv[-1])
    scale = max(scale, float(np.abs(q[..., :3]).max()))
    return {"normal": _unit(_unit(n_obj) @ Mi), "u": u, "residual": np.abs(dist - c0[:, 3]), "radius": c0[:, 3], "kappa": float(sv[0] / sv[-1]),
            "scale": scale, "bend": np.linalg.norm(c2[:, :3], axis=1) / np.linalg.norm(c1[:, :3], axis=1), "speed": np.linalg.norm(c1[:, :3], axis=1)}


def curve_clearance(arr, rays, per_segment=512):
    """how far every ray passes from every strand of every curve instance (type 2): the smallest, over spheres of the sweep at `per_segment` values of u per
    segment, of (distance of the ray's line in front of its origin to the centre - radius) / radius, in object space, float64.  Negative: the ray enters the sweep;
    positive: it misses it.  The sampled union of spheres differs from the envelope of all of them by (spacing of the centres)^2 / (8 r), and the envelope from the
    curve's offset surface by r a^2 / 2 (module docstring): both below 2e-4 r for the strands of these tests, so a pixel whose |clearance| exceeds
    CURVE_EDGE = 1e-3 hits or misses for certain.
    -> (clearance (N,), instance (N,), roughly where along the ray (N,)); inf / -1 where the scene has no curves"""
    o = np.asarray(rays[0], np.float64).reshape(-1, 3)
    d = np.asarray(rays[1], np.float64).reshape(-1, 3)
    best, who, where = np.full(len(o), np.inf), np.full(len(o), -1), np.full(len(o), np.nan)
    us = (np.arange(per_segment) + 0.5) / per_segment
    for i, rec in enumerate(arr["instances"]):
        if int(rec["type"]) != 2:
            continue
        Mx = instance_matrix(arr, i)
        Mi = np.linalg.inv(Mx[:, :3])
        oo, dd = (o - Mx[:, 3]) @ Mi.T, d @ Mi.T
        cu = arr["curves"][int(rec["geom_id"])]
        counts = arr["curve_vertex_counts"][int(cu["vertex_counts_start"]):int(cu["vertex_counts_start"]) + int(cu["vertex_counts_count"])]
        nseg = int(sum(max(int(c) - 3, 0) for c in counts))
        for s in range(nseg):
            c = bspline(segment_control_points(arr, i, np.array([s]))[0][None], us)  # (per_segment, 4)
            rel = c[None, :, :3] - oo[:, None, :]
            tt = np.maximum((rel * dd[:, None, :]).sum(-1) / (dd * dd).sum(-1)[:, None], 0.0)
            dist = np.linalg.norm(rel - tt[..., None] * dd[:, None, :], axis=-1)
            clr = (dist - c[None, :, 3]) / c[None, :, 3]
            j = np.argmin(clr, axis=1)
            m = clr[np.arange(len(o)), j]
            better = m < best
            best, who, where = np.where(better, m, best), np.where(better, i, who), np.where(better, tt[np.arange(len(o)), j], where)
    return best, who, where


CURVE_EDGE = 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def barycentric_error(size_ratio, cos):
    """An fp32 ray / triangle test works on coordinates of magnitude <= L and cannot place the point it finds better than C_ISECT roundings of L, U L each; the
    point's error along the ray shows in the triangle's plane amplified by 1 / cos of the incidence angle.  A displacement e in the plane moves a barycentric
    weight by at most e / (the smallest altitude h): |d weight| <= C_ISECT U (L / h) / cos, size_ratio = L / h."""
    return C_ISECT * U * size_ratio / cos


def direction_bound(kappa, length, spread, size_ratio, cos):
    """Per component, on a world-space unit normal (or tangent: the same chain) taken from the image as 2 pixel - 1:
      the unpacked vertex values are exact (q / 256 - 1);
      the blend n0 w + n1 u + n2 v, w = 1 - u - v: two roundings in w, three products, two sums -- 7 U absolute on components <= 1 -- and the weights' own
        error, 2 barycentric_error spread (n = n0 + u (n1 - n0) + v (n2 - n0); spread = the largest difference of two vertex values): relative to the blended
        vector's length `length`, (7 U + 2 e_b spread) / length;
      the 3 x 3 product with inverse(M3)^T, its entries rounded once from float64: 1 + 3 products + 2 sums = 6 U relative to |inverse(M3)^T| |n|;
      the normalisation divides by a length that may be as small as |n| / sigma_max: what came before is amplified by kappa = sigma_max / sigma_min of M3;
      the normalisation itself: three squares and two sums (3 U on the sum, halved by the root), the root, the reciprocal, the product: 4.5 U;
      (n + 1) / 2 rounds a number <= 2 once, U of 2: 2 U on n; the halving and the test's 2 x - 1 in float64 are exact.
    (16 U kappa for a flat triangle of unit-length normals would be the count to the nearest power of two; this one keeps the terms apart.)"""
    return ((7 * U + 2 * barycentric_error(size_ratio, cos) * spread) / length + 6 * U) * kappa + 6.5 * U


def mapped_bound(e_n, e_t, ts, m_len, texture_error=1e-6):
    """The mapped normal normalize(tu x + tv y + n z), (x, y, z) = 2 texel - 1, per component; e_n, e_t = direction_bound of the normal and of tangent_u.
      tv = cross(n, tu): a component a b - c d of unit vectors off by e_n, e_t moves by <= 2 (e_n + e_t), plus two products and a difference, 3 U;
      a constant texture returns its value within 1e-6 (tests/test_textures.py: the four weights sum to one within their roundings): 2e-6 + U on x, y, z, each
        multiplying a unit vector;
      the sum: three products and two sums, 5 U on components <= |x| + |y| + |z| <= 3, taken as 15 U;
      the normalisation divides by m_len = |tu x + tv y + n z| (tu and n are not orthogonal: the tangent went through the normal transform), then 4.5 U + 2 U as
        for direction_bound."""
    e_tv = 2 * (e_n + e_t) + 3 * U
    e_m = e_t * abs(ts[0]) + e_tv * abs(ts[1]) + e_n * abs(ts[2]) + 3 * (2 * texture_error + U) + 15 * U
    return e_m / m_len + 6.5 * U


def position_bound(scale, cos):
    """Per component of the world-space position M (p0 w + p1 u + p2 v), scale = L = the largest magnitude in the chain (object-space coordinates times the
    matrix's absolute row sums plus the translation, the world-space vertices, the ray origin the intersector saw):
      the blend: 7 roundings (direction_bound) on numbers <= L_object, carried through the matrix: 7 U L;
      the 3 x 4 product: three products and three sums, 6 U L;
      the barycentrics of the fp32 intersector place the point within C_ISECT U L / cos of the float64 point (barycentric_error; cos >= 1/2 in these scenes);
      one more U L for what follows in offset_ray: 256 n truncated to an integer may differ by one step, one ulp of the coordinate."""
    return (7 + 6 + C_ISECT / cos + 2) * U * scale


CURVE_DU = 5e-5  # the curve intersector ends its iteration when a step in u is shorter than this (the product's and the checker's intersect_curve_segment)


def curve_normal_bound(scale, radius, kappa, bend, speed):
    """Per component of a curve's world-space normal.  The normal of a tube of radius r moves by |dp| / r when the point or the axis moves by dp, so every
    absolute error of the object-space chain counts relative to `radius`, r at the hit; L = scale = the largest coordinate magnitude (world-space ones times
    |inverse(M3)|):
      the hit point o + t d: a product and a sum, 2 U L;  to object space: the difference with the translation, U L, and the 3 x 3 product with once-rounded
        entries, 6 U L: 9 U L;
      the centre c(u) and the velocity c'(u): polynomial coefficients from four control points (three products, three sums, a quotient: 7 U L) and Horner's
        rule (three products, three sums: 6 U L): 13 U L each; the velocity enters through the projection (p - c) - ((p - c) . c') c' / |c'|^2, whose error is
        that of a unit vector times |p - c| <= r: counted once more as 13 U L relative to r;
      the assembly of the normal (the projection, the rescaling to r, two products and a difference): 8 U L;
      the parameter u the renderer evaluates c and c' at is the intersector's, not the point's own u*: the intersector stops at u when the step it would take next,
        du, is shorter than CURVE_DU, and reports the point it found on the tangent cone at u, du |c'| further along the axis.  At distance r from an axis of
        curvature |c''| / |c'|^2 that stretch of the axis belongs to a parameter interval of up to du / (1 - r |c''| / |c'|^2) (the outside of a bend), and the
        plane the point is projected to turns with the velocity, by |c''| / |c'| = `bend` per unit of u: CURVE_DU bend / (1 - radius bend / speed) -- not a
        rounding: the one input whose tolerance reaches the normal (the hit's t does not: the point is dropped onto the surface along the radius, and hitref
        judges the normal at that same point);
    43 U (L / radius) + that before the transform, amplified by kappa in the normalisation after it (direction_bound), + 6 U for the product + 6.5 U after."""
    return (43 * U * scale / radius + CURVE_DU * bend / (1.0 - radius * bend / speed) + 6 * U) * kappa + 6.5 * U
