"""Fractional opacity restated on the CPU ("Fractional opacity") -- typed from the definition, not from the device code: the draw in
integer arithmetic (numpy uint32 / uint64 wrap-around), the opacity a = clamp01(fl(fl(scale * texel) + bias)) over tests/mtexref.py's look-up (shared with
tests/cutref.py), the shadow transmittance as the definition's roundings.

The second half builds the small scenes tests/test_gpu_blend.py uses."""
import numpy as np

from strelka_amd import scene as S
from tests import cutref

F = np.float32
U = np.uint32
SALT = 0xB5297A4D


def _u32(x):
    return np.asarray(x).astype(np.uint64) & np.uint64(0xFFFFFFFF)


def murmur(x):
    """hash_murmur (RandomSampler.h:86-95) over uint32 arrays held in uint64"""
    x = _u32(x)
    x ^= x >> np.uint64(16)
    x = _u32(x * np.uint64(0x85EBCA6B))
    x ^= x >> np.uint64(13)
    x = _u32(x * np.uint64(0xC2B2AE35))
    x ^= x >> np.uint64(16)
    return x


def combine(seed, v):
    """hash_combine (RandomSampler.h:50-53)"""
    seed, v = _u32(seed), _u32(v)
    return seed ^ _u32(v + _u32(seed << np.uint64(6)) + (seed >> np.uint64(2)))


def part1by1(x):
    x = _u32(x) & np.uint64(0x0000FFFF)
    x = (x ^ (x << np.uint64(8))) & np.uint64(0x00FF00FF)
    x = (x ^ (x << np.uint64(4))) & np.uint64(0x0F0F0F0F)
    x = (x ^ (x << np.uint64(2))) & np.uint64(0x33333333)
    x = (x ^ (x << np.uint64(1))) & np.uint64(0x55555555)
    return x


def morton2(px, py):
    return _u32((part1by1(py) << np.uint64(1)) + part1by1(px))


def sample_index(px, py, sample, spp_total):
    """the sampler's sampleIdx (init_sampler): encode_morton2(px, py) * sppTotal + pixel sample index, in uint32"""
    return _u32(_u32(morton2(px, py) * _u32(spp_total)) + _u32(sample))


def draw_hash(px, py, sample, spp_total, depth, round_):
    h = murmur(sample_index(px, py, sample, spp_total) ^ np.uint64(SALT))
    return murmur(combine(combine(h, depth), round_))


def xi(px, py, sample, spp_total, depth, round_):
    """(h >> 8) * 2^-24: exact in float32"""
    return ((draw_hash(px, py, sample, spp_total, depth, round_) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(F)


def accepts(a, px, py, sample, spp_total, depth, round_):
    """a radiance ray takes the hit iff xi < a"""
    return xi(px, py, sample, spp_total, depth, round_) < F(a)


def opacity(e, textures, uv):
    """a of an entry (S.MATERIAL_BLEND) at uv: the cutouts' arithmetic"""
    return cutref.opacity(e, textures, uv)


def transmit(contrib, alphas):
    """a shadow ray's contribution after crossing blend hits of opacity alphas (in order of increasing t): w = fl(1 - a), then fl(c * w) per channel"""
    c = np.asarray(contrib, F).copy()
    for a in alphas:
        c = (c * (F(1.0) - F(a)).astype(F)).astype(F)
    return c


def entry(**kw):
    e = np.zeros((), S.MATERIAL_BLEND)
    e["opacity_channel"], e["opacity_scale"], e["active"] = 3, 1.0, 1
    for k, v in kw.items():
        e[k] = v
    return e


def table(n, entries):
    """n materials, `entries` {material: entry(...)}; the others inactive"""
    t = np.zeros(n, S.MATERIAL_BLEND)
    t["opacity_channel"], t["opacity_scale"] = 3, 1.0
    for k, e in entries.items():
        t[k] = e
    return t


def constant(a):
    """an entry of constant opacity a: no texture, scale 0, bias a (fl(0 * 1) + a = a exactly)"""
    return entry(opacity_scale=0.0, opacity_bias=a)
