"""Float64 numpy restatement of the environment light's definition ("Environment light") and the seeded maps the tests use.

Map: (H, W, 3) float32, row 0 = the +Y pole, column 0 at phi = 0 on +X, phi towards +Z.  A world direction d goes through the 3x3 `world_to_env`
rotation, theta = acos(clamp(l.y)), phi = atan2(l.z, l.x) (+ 2 pi if negative), ix = min(int(phi / 2 pi W), W - 1), iy = min(int(theta / pi H), H - 1).
Weight w = luminance_709(texel) sin(pi (iy + 1/2) / H); pdf per solid angle = w / sum w  W H / (2 pi^2 sin theta), sin theta = sqrt(l.x^2 + l.z^2)."""
import numpy as np

LUM = np.array([0.2126, 0.7152, 0.0722])


def sky_map(W, H, seed, sun=True):
    """a smooth gradient (bluish zenith, bright horizon, dark ground) plus, with `sun`, a few texels 10^4 times brighter in the upper hemisphere"""
    rs = np.random.RandomState(seed)
    th = (np.arange(H) + 0.5) / H * np.pi
    ph = (np.arange(W) + 0.5) / W * 2 * np.pi
    up = np.cos(th)[:, None]
    base = np.where(up > 0, 0.3 + 0.7 * (1 - up) ** 3, 0.05 + 0.1 * (1 + up))  # (H, 1)
    tint = np.array(rs.uniform(0.4, 1.0, 3))
    rgb = base[..., None] * (tint[None, None, :] + 0.2 * np.cos(ph[None, :, None] + rs.uniform(0, 6.28, 3)[None, None, :]))
    rgb = np.maximum(rgb, 1e-3)
    if sun:
        iy, ix = int(H * rs.uniform(0.15, 0.35)), int(W * rs.uniform(0.1, 0.9))
        n = max(1, min(3, H // 32))
        rgb[iy:iy + n, ix:ix + n] = rgb[iy:iy + n, ix:ix + n] * 1e4 * np.array([1.0, 0.9, 0.7])
    return np.ascontiguousarray(rgb, np.float32)


def weights(rgb):
    H = rgb.shape[0]
    return (rgb.astype(np.float64) @ LUM) * np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None]


def cdfs(rgb):
    """(marginal CDF with a leading 0: H + 1, conditional CDFs with a leading 0: H x (W + 1), sum w), float64"""
    w = weights(rgb)
    rows = w.sum(axis=1)
    total = rows.sum()
    marg = np.concatenate([[0.0], np.cumsum(rows) / total])
    cond = np.concatenate([np.zeros((len(w), 1)), np.cumsum(w, axis=1) / np.maximum(rows, 1e-300)[:, None]], axis=1)
    return marg, cond, total


def to_env(d, world_to_env=None):
    d = np.asarray(d, np.float64)
    return d if world_to_env is None else d @ np.asarray(world_to_env, np.float64).reshape(3, 3).T


def texel_coords(d, W, H, world_to_env=None):
    """continuous texel coordinates (x in [0, W], y in [0, H]) of world directions, float64"""
    l = to_env(d, world_to_env)
    theta = np.arccos(np.clip(l[:, 1], -1.0, 1.0))
    phi = np.arctan2(l[:, 2], l[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    return phi / (2 * np.pi) * W, theta / np.pi * H


def texel_of(d, W, H, world_to_env=None):
    x, y = texel_coords(d, W, H, world_to_env)
    return np.minimum(x.astype(np.int64), W - 1), np.minimum(y.astype(np.int64), H - 1)


def pdf(rgb, d, ix, iy, world_to_env=None):
    """solid-angle pdf of directions d GIVEN their texel (ix, iy) (the caller decides the texel: edge cases are compared against the neighbour reported)"""
    H, W = rgb.shape[:2]
    w = weights(rgb)
    l = to_env(d, world_to_env)
    st = np.sqrt(l[:, 0] ** 2 + l[:, 2] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = w[iy, ix] / w.sum() * W * H / (2 * np.pi ** 2 * st)
    return np.where((w[iy, ix] > 0) & (st > 0), p, 0.0)


def cosine_moments(rgb, scale=(1, 1, 1)):
    """(E_cos[Le], E_cos[Le^2]) per channel over the upper hemisphere (+Y), cosine-distributed directions, identity rotation: exact for the
    piecewise-constant map -- a texel's share is Integral cos(theta) d omega / pi = (2 pi / W) (sin^2 theta1 - sin^2 theta0) / 2 / pi, theta clipped to pi / 2"""
    H, W = rgb.shape[:2]
    t0 = np.minimum(np.arange(H) / H * np.pi, np.pi / 2)
    t1 = np.minimum((np.arange(H) + 1) / H * np.pi, np.pi / 2)
    share = (np.sin(t1) ** 2 - np.sin(t0) ** 2) / W  # per texel of the row; sums to 1 over the hemisphere
    Le = rgb.astype(np.float64) * np.asarray(scale, np.float64)
    return (Le * share[:, None, None]).sum(axis=(0, 1)), (Le ** 2 * share[:, None, None]).sum(axis=(0, 1))


def random_directions(n, seed):
    rs = np.random.RandomState(seed)
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(d, np.float32)
