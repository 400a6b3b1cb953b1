"""Material textures restated in numpy ("Material textures") -- typed from the definition, not from the device code.
The look-up and resolve_material in float32, operation by operation (the library is built with -ffp-contract=off: bit equality is the bar);
the emission at an emitter sample in float64.  tests/test_mtex_cpu.py holds the look-up against the CPU oracle's, tests/test_gpu_mtex.py the GPU
against all of it."""
import numpy as np

F = np.float32
RGB = 4  # emission_channel: the texel's rgb


def unpack_uv(packed):
    """unpackUV: 16-16 bits over [-10, 10], fp32 arithmetic -> (u, v)"""
    p = np.asarray(packed, np.uint32)
    u = (p & np.uint32(0xFFFF)).astype(F) / F(16383.99999) * F(20.0) - F(10.0)
    v = (p >> np.uint32(16)).astype(F) / F(16383.99999) * F(20.0) - F(10.0)
    return u.astype(F), v.astype(F)


def _axis(c, n):
    """wrap addressing, linear filter: the two texel indices and the 1.8 fixed-point weight of the second"""
    c = np.asarray(c, F)
    x = (c - np.floor(c)) * F(n) - F(0.5)
    fl = np.floor(x)
    a = np.floor((x - fl) * F(256.0) + F(0.5)) * F(1.0 / 256.0)
    i = fl.astype(np.int64)
    i0 = np.where(i < 0, i + n, i) % n
    return i0, (i0 + 1) % n, a.astype(F)


def lookup(tex, uv):
    """tex: (H, W, 4) uint8, rows top to bottom; uv: (n, 2) float32 -> (n, 4) float32: bilinear, wrap, texel = byte / 255, no sRGB decode;
    the sum in the order ((w00 t00 + w10 t10) + w01 t01) + w11 t11"""
    tex = np.asarray(tex, np.uint8)
    uv = np.asarray(uv, F).reshape(-1, 2)
    h, w = tex.shape[:2]
    x0, x1, a = _axis(uv[:, 0], w)
    y0, y1, b = _axis(uv[:, 1], h)
    t = tex.astype(F) / F(255.0)
    t00, t10, t01, t11 = t[y0, x0], t[y0, x1], t[y1, x0], t[y1, x1]
    one = F(1.0)
    w00, w10, w01, w11 = ((one - a) * (one - b))[:, None], (a * (one - b))[:, None], ((one - a) * b)[:, None], (a * b)[:, None]
    return (((w00 * t00 + w10 * t10) + w01 * t01) + w11 * t11).astype(F)


def clamp01(x):
    return np.minimum(np.maximum(np.asarray(x, F), F(0.0)), F(1.0))


def emission_texel(c, channel):
    """(n, 4) texels -> (n, 3): rgb, or one channel for all three"""
    return c[:, :3] if channel == RGB else np.repeat(c[:, channel:channel + 1], 3, axis=1)


def _valid(tid, textures):
    return 0 < int(tid) <= len(textures)


def resolve_material(material, entry, Le, textures, uv):
    """material: one S.MATERIAL record; entry: one S.MATERIAL_TEXTURES record (None: no table); Le: the material's radiance (3,);
    textures: the list skh_set_textures got; uv: (n, 2) -> (n, 8) float32: base_color[3], roughness, metallic, Le[3].
    Texture ids are 1-based, 0 or beyond the list = none.  Roughness / metallic maps apply to PBR materials (type 1) only and a shared id
    is looked up once (the same texel either way); value = clamp01(fl(fl(scale * texel) + bias)).  Le = Le_material * texel."""
    uv = np.asarray(uv, F).reshape(-1, 2)
    n = len(uv)
    out = np.zeros((n, 8), F)
    out[:, 0:3] = np.asarray(material["base_color"], F)
    out[:, 3], out[:, 4] = F(material["roughness"]), F(material["metallic"])
    out[:, 5:8] = np.asarray(Le, F)
    if _valid(material["base_color_texture"], textures):
        out[:, 0:3] = lookup(textures[int(material["base_color_texture"]) - 1], uv)[:, :3]
    if entry is None:
        return out
    if int(material["type"]) == 1:
        for col, slot in ((3, "roughness"), (4, "metallic")):
            if _valid(entry[slot + "_texture"], textures):
                t = lookup(textures[int(entry[slot + "_texture"]) - 1], uv)[:, int(entry[slot + "_channel"])]
                prod = (F(entry[slot + "_scale"]) * t).astype(F)
                out[:, col] = clamp01((prod + F(entry[slot + "_bias"])).astype(F))
    if _valid(entry["emission_texture"], textures) and (np.asarray(Le, F) > 0).any():
        c = lookup(textures[int(entry["emission_texture"]) - 1], uv)
        out[:, 5:8] = (np.asarray(Le, F)[None, :] * emission_texel(c, int(entry["emission_channel"]))).astype(F)
    return out


def lookup64(tex, uv):
    """the same filter in float64 (the weights are still 1.8 fixed point: that is the definition, not a rounding)"""
    tex = np.asarray(tex, np.uint8)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    h, w = tex.shape[:2]

    def axis(c, n):
        x = (c - np.floor(c)) * n - 0.5
        fl = np.floor(x)
        a = np.floor((x - fl) * 256.0 + 0.5) / 256.0
        i0 = fl.astype(np.int64) % n
        return i0, (i0 + 1) % n, a

    x0, x1, a = axis(uv[:, 0], w)
    y0, y1, b = axis(uv[:, 1], h)
    t = tex.astype(np.float64) / 255.0
    a, b = a[:, None], b[:, None]
    return (1 - a) * (1 - b) * t[y0, x0] + a * (1 - b) * t[y0, x1] + (1 - a) * b * t[y1, x0] + a * b * t[y1, x1]


def emission_at_sample(Le, tex, channel, tri_uv, ux, uy):
    """float64: Le(x) = Le_material * texel at the sampled point of a triangle whose vertices carry tri_uv (..., 3, 2): the barycentrics of the
    uniform-by-area point, (1 - sqrt ux, sqrt ux (1 - uy), sqrt ux uy)"""
    su = np.sqrt(np.asarray(ux, np.float64))
    uy = np.asarray(uy, np.float64)
    b = np.stack([1 - su, su * (1 - uy), su * uy], -1)
    uv = (b[..., None] * np.asarray(tri_uv, np.float64)).sum(-2)
    return np.asarray(Le, np.float64) * emission_texel(lookup64(tex, uv), channel)


def neighbour_difference(tex, channels):
    """D: the largest difference, as a fraction of 255, between a texel and a neighbour (the next column, the next row, with wrap) in `channels`"""
    t = np.asarray(tex, np.float64)[..., channels] / 255.0
    return float(max(np.abs(t - np.roll(t, 1, axis=0)).max(), np.abs(t - np.roll(t, 1, axis=1)).max()))
