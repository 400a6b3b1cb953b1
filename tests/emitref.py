"""Emissive meshes restated in numpy float64 ("Emissive meshes"): the emitter table, the selection, the point on the
triangle, the pdf, and Lambert's polygon formula for the irradiance under a uniform polygonal emitter -- typed from the definition, not from
the device code.  tests/test_emit_cpu.py holds it against quadrature and a one-triangle closed form, tests/test_gpu_emit.py the GPU against it."""
import numpy as np

LUM = np.array([0.2126, 0.7152, 0.0722])


def lum709(Le):
    return np.asarray(Le, np.float64) @ LUM


def world_triangles(tris, M=None):
    """tris: (N, 3, 3) object-space vertices; M: 3x4 (or 4x4) object -> world.  Float64 from whatever precision the inputs have."""
    t = np.asarray(tris, np.float64)
    if M is None:
        return t
    M = np.asarray(M, np.float64)
    return t @ M[:3, :3].T + M[:3, 3]


def areas(world):
    return 0.5 * np.linalg.norm(np.cross(world[:, 1] - world[:, 0], world[:, 2] - world[:, 0]), axis=1)


def table(world, lum):
    """-> (weights w_k = area_k * lum_k, inclusive CDF, sum w)"""
    w = areas(world) * np.asarray(lum, np.float64)
    c = np.cumsum(w)
    return w, c / c[-1], float(c[-1])


def select(cdf, u):
    """smallest k with u < cdf[k], at most N - 1"""
    return np.minimum(np.searchsorted(cdf, np.asarray(u, np.float64), side="right"), len(cdf) - 1)


def point(tri, ux, uy):
    """tri: (..., 3, 3); uniform by area: su = sqrt(ux), p = (1 - su) v0 + su (1 - uy) v1 + su uy v2"""
    su = np.sqrt(np.asarray(ux, np.float64))[..., None]
    uy = np.asarray(uy, np.float64)[..., None]
    return (1 - su) * tri[..., 0, :] + su * (1 - uy) * tri[..., 1, :] + su * uy * tri[..., 2, :]


def normal(tri, flip=False):
    """the emitting side: the world winding's normal, turned round (`flip`) when the instance transform mirrors"""
    n = np.cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :])
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    return -n if flip else n


def pdf(n_e, lum, sum_w, x, origin):
    """per solid angle at `origin` of the point x on an emitter of normal n_e and luminance lum: lum / sum w * dist^2 / cos_e; 0 from behind"""
    d = np.asarray(x, np.float64) - np.asarray(origin, np.float64)
    dist = np.linalg.norm(d, axis=-1)
    cos_e = -(d * n_e).sum(-1) / dist
    return np.where(cos_e > 0, np.asarray(lum, np.float64) / sum_w * dist ** 2 / np.where(cos_e > 0, cos_e, 1.0), 0.0)


def polygon_irradiance(poly, p, n):
    """Lambert's formula: E / Le at the point p with normal n under a uniform Lambertian polygon that lies wholly above p's horizon:
    1/2 |sum_i gamma_i n . unit(v_i x v_i+1)| over the unit vectors v_i from p to the vertices, gamma_i the angle between v_i and v_i+1."""
    v = np.asarray(poly, np.float64) - np.asarray(p, np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    w = np.roll(v, -1, axis=0)
    c = np.cross(v, w)
    s = np.linalg.norm(c, axis=1)
    gamma = np.arctan2(s, (v * w).sum(1))
    return 0.5 * abs(float((gamma * (c @ np.asarray(n, np.float64)) / s).sum()))


def quad_irradiance_quadrature(corner, ex, ey, p, n, m=2000):
    """the same by the midpoint rule over m x m cells of the parallelogram corner + s ex + t ey: E / Le = integral of cos cos' / r^2 dA"""
    corner, ex, ey, p, n = [np.asarray(a, np.float64) for a in (corner, ex, ey, p, n)]
    s = (np.arange(m) + 0.5) / m
    X = corner[None, None, :] + s[:, None, None] * ex[None, None, :] + s[None, :, None] * ey[None, None, :]
    ne = np.cross(ex, ey)
    dA = np.linalg.norm(ne) / (m * m)
    ne = ne / np.linalg.norm(ne)
    d = X - p
    r2 = (d * d).sum(-1)
    cos_p = (d @ n) / np.sqrt(r2)
    cos_e = np.abs(d @ ne) / np.sqrt(r2)
    return float((np.maximum(cos_p, 0) * cos_e / r2).sum() * dA)


def weight_error_bound(world, lum, U=2.0 ** -24):
    """Bound on |w32_k - w_k| for a weight evaluated in fp32 (half-ulp U per operation) from world-space vertices that ARE exact fp32 numbers with exact
    differences: a cross-product component a b - c d carries U (|a b| + |c d|) + U |a b - c d|, so the cross product's length is off by at most
    U (|e1|_1 |e2|_1 + |c|); the three squares, two sums, the root, the product by 1/2 and the product by the (once-rounded) luminance add 9 U relative."""
    e1, e2 = world[:, 1] - world[:, 0], world[:, 2] - world[:, 0]
    c = np.linalg.norm(np.cross(e1, e2), axis=1)
    return np.asarray(lum, np.float64) * (0.5 * U * (np.abs(e1).sum(1) * np.abs(e2).sum(1) + c) + 9 * U * 0.5 * c)
