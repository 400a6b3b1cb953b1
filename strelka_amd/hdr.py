"""Minimal Radiance `.hdr` (RGBE) reader / writer: the file format lat-long environment maps come in.

Reader: `#?RADIANCE` / `#?RGBE` header, `FORMAT=32-bit_rle_rgbe`, resolution line `-Y H +X W` (the standard top-to-bottom, left-to-right
orientation; others are refused), scanlines flat or new-style run-length encoded (Ward, "Real Pixels", Graphics Gems II; the per-channel
RLE of Radiance 2.0: 2 2 hi lo, then each of the four byte planes as runs > 128 / literals <= 128).  Old-style RLE (a (1, 1, 1, n) repeat
pixel) is not decoded: such a pixel reads as the dark grey it also spells.  Result: (H, W, 3) float32, row 0 = the top of the picture = the +Y pole of `Scene.setEnvironment`'s convention.
Writer: the same, RLE (default, widths 8..32767) or flat.  A value is stored as a shared exponent and three 8-bit mantissas
(`rgbe_quantise` is what survives the round trip); EXPOSURE lines are ignored.
"""
import re

import numpy as np


class HdrError(ValueError):
    pass


def float_to_rgbe(rgb):
    """(..., 3) non-negative floats -> (..., 4) uint8: mantissa = floor(v * 256 / 2^e), e = the exponent of the largest channel (frexp)"""
    rgb = np.asarray(rgb, np.float32)
    if not np.isfinite(rgb).all() or (rgb < 0).any():
        raise HdrError("RGBE holds finite non-negative values only")
    v = rgb.max(axis=-1)
    m, e = np.frexp(v)  # v = m * 2^e, 0.5 <= m < 1
    out = np.zeros(rgb.shape[:-1] + (4,), np.uint8)
    ok = v >= 1e-32
    scale = np.where(ok, np.ldexp(np.float64(256.0), -e.astype(np.int64)), 0.0)  # 256 / 2^e
    out[..., :3] = np.minimum(np.floor(rgb.astype(np.float64) * scale[..., None]), 255).astype(np.uint8)
    out[..., 3] = np.where(ok, e + 128, 0).astype(np.uint8)
    out[~ok] = 0
    return out


def rgbe_to_float(rgbe):
    """(..., 4) uint8 -> (..., 3) float32: (mantissa + 0.5) * 2^(e - 136), 0 where e = 0 (Radiance's colr_color)"""
    rgbe = np.asarray(rgbe, np.uint8)
    e = rgbe[..., 3].astype(np.int64)
    f = np.ldexp(np.float64(1.0), e - 136)
    out = (rgbe[..., :3].astype(np.float64) + 0.5) * f[..., None]
    out[e == 0] = 0.0
    return out.astype(np.float32)


def rgbe_quantise(rgb):
    """what a write + read of `rgb` gives back"""
    return rgbe_to_float(float_to_rgbe(rgb))


def _rle_plane(row):
    """one byte plane of a scanline -> new-style runs: (128 + n, value) for n >= 3 equal bytes, (n, literals) otherwise, n <= 127 / 128"""
    out = bytearray()
    n, i = len(row), 0
    while i < n:
        run = 1
        while i + run < n and run < 127 and row[i + run] == row[i]:
            run += 1
        if run >= 3:
            out += bytes((128 + run, row[i]))
            i += run
            continue
        j = i  # literal stretch up to the next run of >= 3
        while j < n and j - i < 128:
            r = 1
            while j + r < n and r < 3 and row[j + r] == row[j]:
                r += 1
            if r >= 3:
                break
            j += 1
        out += bytes((j - i,)) + bytes(row[i:j])
        i = j
    return bytes(out)


def encode_hdr(rgb, rle=True):
    rgb = np.asarray(rgb, np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise HdrError("an (H, W, 3) image is expected")
    h, w = rgb.shape[:2]
    px = float_to_rgbe(rgb)
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode()
    if not rle or w < 8 or w > 32767:
        return head + px.tobytes()
    body = bytearray()
    for y in range(h):
        body += bytes((2, 2, w >> 8, w & 255))
        for c in range(4):
            body += _rle_plane(px[y, :, c].tolist())
    return head + bytes(body)


def save_hdr(path, rgb, rle=True):
    with open(path, "wb") as f:
        f.write(encode_hdr(rgb, rle))


def decode_hdr(data, name="<bytes>"):
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
        raise HdrError(f"{name}: not a Radiance picture (no #?RADIANCE signature)")
    end = data.find(b"\n\n")
    if end < 0:
        raise HdrError(f"{name}: the header does not end")
    header = data[:end].decode("latin-1").split("\n")
    fmt = [ln.split("=", 1)[1].strip() for ln in header if ln.startswith("FORMAT=")]
    if fmt != ["32-bit_rle_rgbe"]:
        raise HdrError(f"{name}: FORMAT must be 32-bit_rle_rgbe, found {fmt}")
    eol = data.find(b"\n", end + 2)
    if eol < 0:
        raise HdrError(f"{name}: no resolution line")
    m = re.fullmatch(r"-Y (\d+) \+X (\d+)", data[end + 2:eol].decode("latin-1").strip())
    if not m:
        raise HdrError(f"{name}: only the standard orientation '-Y H +X W' is read")
    h, w = int(m.group(1)), int(m.group(2))
    if h < 1 or w < 1 or h * w > (1 << 28):
        raise HdrError(f"{name}: unreasonable size {w} x {h}")
    buf = memoryview(data)[eol + 1:]
    px = np.zeros((h, w, 4), np.uint8)
    pos = 0
    for y in range(h):
        if 8 <= w <= 32767 and len(buf) >= pos + 4 and buf[pos] == 2 and buf[pos + 1] == 2 and (buf[pos + 2] << 8 | buf[pos + 3]) == w:
            pos += 4
            for c in range(4):
                x = 0
                while x < w:
                    if pos >= len(buf):
                        raise HdrError(f"{name}: truncated in scanline {y}")
                    n = buf[pos]
                    pos += 1
                    if n > 128:
                        n -= 128
                        if pos >= len(buf) or x + n > w:
                            raise HdrError(f"{name}: bad run in scanline {y}")
                        px[y, x:x + n, c] = buf[pos]
                        pos += 1
                    else:
                        if n == 0 or pos + n > len(buf) or x + n > w:
                            raise HdrError(f"{name}: bad literal stretch in scanline {y}")
                        px[y, x:x + n, c] = np.frombuffer(buf[pos:pos + n], np.uint8)
                        pos += n
                    x += n
        else:
            if len(buf) < pos + 4 * w:
                raise HdrError(f"{name}: truncated in scanline {y}")
            row = np.frombuffer(buf[pos:pos + 4 * w], np.uint8).reshape(w, 4)
            px[y] = row
            pos += 4 * w
    return rgbe_to_float(px)


def load_hdr(path):
    with open(path, "rb") as f:
        return decode_hdr(f.read(), path)
