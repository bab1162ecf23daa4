"""Packed 10 / 12-bit camera samples in plain numpy: the yardstick of the packed-format tests.

A packed frame is rows of bit-packed samples, a uint8 array [h][row bytes or more].  B[k] is byte k of a row, v(x) pixel x's sample:

    MIPI10 (CSI-2 RAW10)   4 px in 5 bytes, g = x >> 2, i = x & 3    v = B[5g+i] << 2 | ((B[5g+4] >> 2i) & 3)     5 * ceil(w / 4) bytes
    MIPI12 (CSI-2 RAW12)   2 px in 3 bytes, g = x >> 1, i = x & 1    v = B[3g+i] << 4 | ((B[3g+2] >> 4i) & 15)    3 * ceil(w / 2)
    P10 (PFNC Mono10p)     the row is one little-endian bit stream   v = bits [10x, 10x + 10)                     ceil(10 w / 8)
    P12 (PFNC Mono12p)     the same                                  v = bits [12x, 12x + 12)                     ceil(12 w / 8)

`pack` and `unpack` are written from this table and nothing else.  What a packed frame means comes from the models that were here
before: its samples written as little-endian 16-bit values are a GRAY16 (tests/pixfmt_model.py) or BAYER_<pattern>16
(tests/bayer_model.py) frame with bits = 10 / 12, scaled by tests/scale_model.py -- no reduction arithmetic of its own."""
import numpy as np

from tests import bayer_model as bm
from tests import pixfmt_model as pm
from tests import scale_model as sm

MIPI10, MIPI12, P10, P12 = PACKINGS = ("mipi10", "mipi12", "p10", "p12")   # in format-number order
BITS = {MIPI10: 10, MIPI12: 12, P10: 10, P12: 12}
_SUFFIX = {MIPI10: "10_mipi", MIPI12: "12_mipi", P10: "10p", P12: "12p"}
_PATTERNS = ("rggb", "grbg", "gbrg", "bggr")

MONO = tuple(range(32, 36))      # GRAY10_MIPI, GRAY12_MIPI, GRAY10P, GRAY12P
BAYER = tuple(range(40, 56))     # 40 + 4 * packing + pattern
FORMATS = MONO + BAYER
PACKING = {32 + p: k for p, k in enumerate(PACKINGS)}
PACKING.update({40 + 4 * p + q: k for p, k in enumerate(PACKINGS) for q in range(4)})
NAMES = {32 + p: "gray" + _SUFFIX[k] for p, k in enumerate(PACKINGS)}
NAMES.update({40 + 4 * p + q: "bayer_%s%s" % (_PATTERNS[q], _SUFFIX[k]) for p, k in enumerate(PACKINGS) for q in range(4)})
# the unpacked counterpart: GRAY16 or BAYER_<pattern>16
UNPACKED = {f: pm.GRAY16 for f in MONO}
UNPACKED.update({f: bm.RGGB16 + ((f - 40) & 3) for f in BAYER})


def row_bytes(w, packing):
    if packing == MIPI10:
        return 5 * ((w + 3) // 4)
    if packing == MIPI12:
        return 3 * ((w + 1) // 2)
    return (BITS[packing] * w + 7) // 8


def pack(samples, packing):
    """samples [h][w] (integers below 2^bits) -> uint8 [h][row_bytes(w)]; the bits no sample owns are zero"""
    s = np.asarray(samples).astype(np.int64)
    h, w = s.shape
    bits = BITS[packing]
    assert s.min(initial=0) >= 0 and s.max(initial=0) < (1 << bits)
    out = np.zeros((h, row_bytes(w, packing)), np.int64)
    x = np.arange(w)
    if packing == MIPI10:
        g, i = x >> 2, x & 3
        out[:, 5 * g + i] = s >> 2
        np.bitwise_or.at(out, (slice(None), 5 * g + 4), (s & 3) << (2 * i))
    elif packing == MIPI12:
        g, i = x >> 1, x & 1
        out[:, 3 * g + i] = s >> 4
        np.bitwise_or.at(out, (slice(None), 3 * g + 2), (s & 15) << (4 * i))
    else:   # one little-endian bit stream: bit k of sample x is bit bits * x + k of the row
        stream = np.zeros((h, out.shape[1] * 8), np.int64)
        for k in range(bits):
            stream[:, bits * x + k] = (s >> k) & 1
        out = (stream.reshape(h, -1, 8) << np.arange(8)).sum(-1)
    return out.astype(np.uint8)


def unpack(rows, w, packing):
    """uint8 [h][>= row_bytes(w)] -> the samples [h][w] int64"""
    assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.shape[1] >= row_bytes(w, packing), (rows.shape, w, packing)
    B = rows.astype(np.int64)
    x = np.arange(w)
    if packing == MIPI10:
        g, i = x >> 2, x & 3
        return B[:, 5 * g + i] << 2 | ((B[:, 5 * g + 4] >> (2 * i)) & 3)
    if packing == MIPI12:
        g, i = x >> 1, x & 1
        return B[:, 3 * g + i] << 4 | ((B[:, 3 * g + 2] >> (4 * i)) & 15)
    bits = BITS[packing]
    stream = (B[:, :, None] >> np.arange(8)) & 1          # [h][bytes][8], lsb first
    stream = stream.reshape(B.shape[0], -1)
    v = np.zeros((B.shape[0], w), np.int64)
    for k in range(bits):
        v |= stream[:, bits * x + k] << k
    return v


def as16(samples):
    """samples [h][w] -> the unpacked frame [h][w][2]: little-endian 16-bit values"""
    return pm.samples16(samples)


def frame16(rows, w, fmt):
    return as16(unpack(rows, w, PACKING[fmt]))


def reduce(rows, w, fmt, limited_range=0):
    """A packed frame -> the gray plane [h][w] uint8 of its unpacked counterpart"""
    bits = BITS[PACKING[fmt]]
    if fmt in MONO:
        return pm.reduce(frame16(rows, w, fmt), pm.GRAY16, bits, limited_range)
    assert not limited_range
    return bm.reduce(frame16(rows, w, fmt), UNPACKED[fmt], bits)


def scale(rows, geo, W, H, fmt, limited_range=0):
    """A packed frame of geo = (src_width, src_height, crop_x, crop_y, cw, ch) -> the W x H plane of its unpacked counterpart"""
    bits = BITS[PACKING[fmt]]
    px = frame16(rows, geo[0], fmt)
    if fmt in MONO:
        return sm.scale(px, geo, W, H, pm.GRAY16, bits, limited_range)
    assert not limited_range
    return bm.scale(px, geo, W, H, UNPACKED[fmt], bits)


def padded(rows, pad, seed=7):
    """The same rows, `pad` bytes of seeded noise after each: a 2-d view of a wider buffer"""
    if pad == 0:
        return np.ascontiguousarray(rows)
    h, n = rows.shape
    buf = np.random.RandomState(seed).randint(0, 256, size=(h, n + pad), dtype=np.uint8)
    buf[:, :n] = rows
    return buf[:, :n]


def needed_bytes(w, h, stride, packing, x0=0, y0=0):
    """first to one past the last byte of the frame's buffer that holds a sample of columns x0 .. x0 + w - 1 of rows y0 .. y0 + h - 1"""
    return stride * (y0 + h - 1) + row_bytes(x0 + w, packing)


def random_samples(w, h, packing, seed):
    return np.random.RandomState(seed).randint(0, 1 << BITS[packing], size=(h, w))
