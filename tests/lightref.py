"""Light shapes in numpy float64: the definition the HIP code (strelka_amd/csrc/skh_lshape.h, the LSHAPE builds of k_shade) is held against.
DESIGN.md section 2, "Light shapes".  No GPU, no shared code with the implementation.

The sampled disk is the 16-gon rays can hit: v_k = O + cos(2 pi k / 16) X + sin(2 pi k / 16) Y, area 8 sin(pi / 8) |X x Y|, unit normal n.  The cone scales a
light's emission by s(c), c = dot(axis, w), w the unit direction from the light point to the shaded point.  The estimator k_shade runs -- the rect light's
protocol: light sampling with lrad = Li cos_s and the balance heuristic against the BSDF's pdf, BSDF sampling with Li cos_l at the proxy hit -- has, on a
Lambertian floor of albedo rho that nothing reflects back to, the per-pixel expectation

    mu(p) = (rho Li / pi) * integral over the light of  s * cos_s [ w_L cos_s + w_B cos_l ] cos_l / d^2  dA
    w_L = p_L / (p_L + p_B), w_B = 1 - w_L,   p_L = d^2 / (cos_l A) / numPick,   p_B = cos_s / pi

(first term: E over the pick and the area of lrad * bsdf / p_L * w_L with bsdf = rho cos_s / pi; second: E over the cosine-distributed direction of
rho * Li cos_l * w_B).  A disk WITHOUT the flag is never sampled and its hit uses the normal scaled by the radius r, with weight 1:
mu = (rho Li / pi) * integral of cos_s * r cos_l * cos_l / d^2 dA."""
import numpy as np

SECTORS = 16


def s_cone(c, cos_outer, cos_inner, focus):
    """s(c) = 0 unless c > cos_outer; t = min((c - cos_outer) / (cos_inner - cos_outer), 1), 1 for a hard edge; s = t^2 (3 - 2 t) * (focus > 0 ? max(c, 0)^focus : 1)"""
    c = np.asarray(c, np.float64)
    if cos_inner > cos_outer:
        t = np.minimum((c - cos_outer) / (cos_inner - cos_outer), 1.0)
    else:
        t = np.ones_like(c)
    s = t * t * (3.0 - 2.0 * t)
    if focus > 0:
        s = s * np.maximum(c, 0.0) ** focus
    return np.where(c > cos_outer, s, 0.0)


def sector(ux):
    """k = min(int(16 ux), 15), u' = 16 ux - k"""
    ux = np.asarray(ux, np.float64)
    k = np.minimum((SECTORS * ux).astype(np.int64), SECTORS - 1)
    return k, SECTORS * ux - k


def disc_vertices(O, X, Y):
    """(17, 3): v_0 ... v_16 = v_0"""
    a = 2.0 * np.pi * np.arange(SECTORS + 1) / SECTORS
    return np.asarray(O, np.float64) + np.cos(a)[:, None] * np.asarray(X, np.float64) + np.sin(a)[:, None] * np.asarray(Y, np.float64)


def disc_area(X, Y):
    return 8.0 * np.sin(np.pi / 8.0) * np.linalg.norm(np.cross(np.asarray(X, np.float64), np.asarray(Y, np.float64)))


def disc_point(O, X, Y, ux, uy):
    """the point the draw (ux, uy) selects: sector k, then uniform by area in (O, v_k, v_k+1): su = sqrt(u'), (1 - su) O + su (1 - uy) v_k + su uy v_k+1"""
    k, up = sector(ux)
    v = disc_vertices(O, X, Y)
    su = np.sqrt(up)[:, None]
    uy = np.asarray(uy, np.float64)[:, None]
    return (1.0 - su) * np.asarray(O, np.float64) + su * (1.0 - uy) * v[k] + su * uy * v[k + 1]


def area_pdf(n, area, x, P):
    """per solid angle at P of the point x on a light of unit normal n and area A: d^2 / (cos_l A); 0 from behind"""
    d = np.asarray(x, np.float64) - np.asarray(P, np.float64)
    dist = np.linalg.norm(d, axis=-1)
    cos_l = -(d * n).sum(-1) / dist
    return np.where(cos_l > 0, dist * dist / (np.where(cos_l > 0, cos_l, 1.0) * area), 0.0)


def triangle_cells(tris, m):
    """midpoint (centroid) rule: every triangle of tris (T, 3, 3) split into m^2 congruent ones -> (T m^2, 3) centroids, (T m^2,) areas"""
    tris = np.asarray(tris, np.float64)
    bary = []
    for i in range(m):
        for j in range(m - i):
            bary.append(((i + 1 / 3) / m, (j + 1 / 3) / m))  # upright cells
            if j < m - i - 1:
                bary.append(((i + 2 / 3) / m, (j + 2 / 3) / m))  # inverted cells
    b = np.array(bary)
    assert len(b) == m * m
    a, e1, e2 = tris[:, None, 0], (tris[:, 1] - tris[:, 0])[:, None], (tris[:, 2] - tris[:, 0])[:, None]
    pts = a + b[None, :, 0, None] * e1 + b[None, :, 1, None] * e2
    area = 0.5 * np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1) / (m * m)
    return pts.reshape(-1, 3), np.repeat(area, m * m)


def disc_cells(O, X, Y, m=24):
    v = disc_vertices(O, X, Y)
    tris = np.stack([np.broadcast_to(np.asarray(O, np.float64), (SECTORS, 3)), v[:-1], v[1:]], 1)
    return triangle_cells(tris, m)


def rect_cells(points, m=96):
    """the rect light p0 + u (p1 - p0) + v (p3 - p0): m x m midpoint cells"""
    p = np.asarray(points, np.float64)[:, :3]
    e1, e2 = p[1] - p[0], p[3] - p[0]
    u = (np.arange(m) + 0.5) / m
    pts = p[0] + u[:, None, None] * e1 + u[None, :, None] * e2
    return pts.reshape(-1, 3), np.full(m * m, np.linalg.norm(np.cross(e1, e2)) / (m * m))


def shape_s(shape, w):
    """s for unit directions w (light point -> shaded point); 1 without a cone.  shape: None or (cos_outer, cos_inner, focus, axis)"""
    if shape is None:
        return np.ones(w.shape[:-1])
    co, ci, focus, axis = shape
    return s_cone((w * np.asarray(axis, np.float64)).sum(-1), co, ci, focus)


def irradiance_quadrature(pts, dA, n, p, N):
    """the pure form factor: integral of cos_s cos_l / d^2 dA (what Lambert's polygon formula gives in closed form)"""
    d = pts - np.asarray(p, np.float64)
    dist = np.linalg.norm(d, axis=1)
    L = d / dist[:, None]
    cos_s, cos_l = np.maximum(L @ np.asarray(N, np.float64), 0.0), np.maximum(-(L @ np.asarray(n, np.float64)), 0.0)
    return float((cos_s * cos_l / dist ** 2 * dA).sum())


def area_light_mu(pts, dA, n, area, p, N, num_pick, shape=None, sampled=True, hit_scale=1.0):
    """mu(p) / (rho Li): the integrand of the module's docstring over quadrature cells (pts, dA) of a flat light of unit normal n and area A.
    sampled = False: the light is never sampled, its hit has weight 1 and the cosine hit_scale * cos_l (the unflagged disk: hit_scale = radius)"""
    d = pts - np.asarray(p, np.float64)
    dist = np.linalg.norm(d, axis=1)
    L = d / dist[:, None]
    cos_s, cos_l = np.maximum(L @ np.asarray(N, np.float64), 0.0), np.maximum(-(L @ np.asarray(n, np.float64)), 0.0)
    s = shape_s(shape, -L)
    ok = (cos_s > 0) & (cos_l > 0)
    cs, cl = np.where(ok, cos_s, 1.0), np.where(ok, cos_l, 1.0)
    if sampled:
        p_l, p_b = dist ** 2 / (cl * area) / num_pick, cs / np.pi
        w_l = p_l / (p_l + p_b)
        f = cs * (w_l * cs + (1.0 - w_l) * cl) * cl / dist ** 2
    else:
        f = cs * (hit_scale * cl) * cl / dist ** 2
    return float((np.where(ok, f * s, 0.0) * dA).sum() / np.pi)


def sphere_light_mu(centre, radius, proxy_tris, p, N, num_pick, shape=None, m_dir=192, m_tri=2):
    """mu(p) / (rho Li) under a sphere light, by the reference's protocol (Lights.h:335-362, get_light_pdf: 1 / 4 pi): the sampler draws a point x uniformly over
    the WHOLE analytic sphere and calls 1 / (4 pi) its pdf per solid angle, lrad = Li cos_s, the front tests dot(N, L) > 0 and -dot(L, n_x) > 0;
    a BSDF ray meets the PROXY (a convex polyhedron, proxy_tris (T, 3, 3) in world space) and adds Li * -dot(rayD, normalize(hit - centre)).
        light sampling: (1 / pi) * integral over the unit sphere of directions u (x = c + r u) of  [front] s cos_s^2 w_L du,  p_L = 1 / (4 pi numPick)
        BSDF sampling:  (1 / pi) * integral over the proxy's faces that face p of  s cos_s cos_l' w_B cos_g / d^2 dA   (cos_g: the face's own cosine)"""
    c, N = np.asarray(centre, np.float64), np.asarray(N, np.float64)
    p = np.asarray(p, np.float64)
    # directions: midpoint rule in (cos theta, phi), equal solid angles
    ct = (np.arange(m_dir) + 0.5) / m_dir * 2.0 - 1.0
    ph = (np.arange(2 * m_dir) + 0.5) / (2 * m_dir) * 2.0 * np.pi
    st = np.sqrt(1.0 - ct * ct)
    u = np.stack([st[:, None] * np.cos(ph), st[:, None] * np.sin(ph), np.broadcast_to(ct[:, None], (m_dir, 2 * m_dir))], -1).reshape(-1, 3)
    dw = 4.0 * np.pi / len(u)
    d = c + radius * u - p
    dist = np.linalg.norm(d, axis=1)
    L = d / dist[:, None]
    cos_s, cos_l = L @ N, -(L * u).sum(1)
    ok = (cos_s > 0) & (cos_l > 0)
    p_l, p_b = 1.0 / (4.0 * np.pi * num_pick), np.where(ok, cos_s, 1.0) / np.pi
    nee = (np.where(ok, shape_s(shape, -L) * cos_s ** 2 * p_l / (p_l + p_b), 0.0)).sum() * dw
    pts, dA = triangle_cells(proxy_tris, m_tri)
    t = np.asarray(proxy_tris, np.float64)
    ng = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ng = ng / np.maximum(np.linalg.norm(ng, axis=1), 1e-300)[:, None]
    ng = np.where(((t.mean(1) - c) * ng).sum(1)[:, None] < 0, -ng, ng)  # outward
    ng = np.repeat(ng, m_tri * m_tri, axis=0)
    d = pts - p
    dist = np.linalg.norm(d, axis=1)
    L = d / dist[:, None]
    ns = (pts - c) / np.linalg.norm(pts - c, axis=1)[:, None]
    cos_s, cos_g, cos_h = L @ N, -(L * ng).sum(1), -(L * ns).sum(1)
    ok = (cos_s > 0) & (cos_g > 0) & (cos_h > 0)
    p_b = np.where(ok, cos_s, 1.0) / np.pi
    hit = (np.where(ok, shape_s(shape, -L) * cos_s * cos_h * (p_b / (p_l + p_b)) * cos_g / dist ** 2, 0.0) * dA).sum()
    return float((nee + hit) / np.pi)


def proxy_triangles(arrays, light_id):
    """world-space triangles (T, 3, 3) of the proxy mesh of light `light_id`, from Scene.arrays()"""
    inst = [i for i in arrays["instances"] if i["type"] == 1 and i["light_id"] == light_id][0]
    me = arrays["meshes"][inst["geom_id"]]
    idx = arrays["indices"][int(me["index_offset"]):int(me["index_offset"]) + int(me["index_count"])].reshape(-1, 3).astype(np.int64)
    pos = arrays["vertices"]["pos"][int(me["vertex_offset"]):int(me["vertex_offset"]) + int(me["vertex_count"])].astype(np.float64)
    M = inst["transform"].astype(np.float64).reshape(3, 4)
    w = pos @ M[:, :3].T + M[:, 3]
    return w[idx]


def shape_of(entry):
    """lightref's shape tuple of an S.LIGHT_SHAPE record, None without a cone"""
    if not (int(entry["flags"]) & 2):
        return None
    return float(entry["cos_outer"]), float(entry["cos_inner"]), float(entry["focus"]), np.asarray(entry["axis"], np.float64)
