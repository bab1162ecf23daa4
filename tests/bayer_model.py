"""Bayer raw mosaics to gray in plain numpy: the yardstick of the Bayer tests.

A mosaic is a uint8 array [..., h, w, bytes per sample] (1 for the *8 formats, 2 for *16: little endian; rows may be strided).  The
format's name gives the colours of the top-left 2 x 2 tile read row by row (GenICam / V4L2 / ROS): RGGB means (0,0) red, (1,0) green,
(0,1) green, (1,1) blue.  A pattern is a phase (px, py) of RGGB -- GRBG (1,0), GBRG (0,1), BGGR (1,1) -- and the colour site of
(x, y) is RGGB's at ((x + px) & 1, (y + py) & 1).

    sample      *8: the byte;  *16: v = b0 | b1 << 8, bits in 8..16 (0 means 16), s = min(255, v >> (bits - 8))
    neighbours  outside the frame mirror without repeating the edge: -1 -> 1, n -> n - 2 (numpy's pad mode 'reflect')
    sums        C = 4 s(x,y);  P = left + right + up + down;  X = the four diagonals;  Hh = 2 (left + right);  Vv = 2 (up + down)
    red site    R4 = C,  G4 = P, B4 = X           green between reds in its row    R4 = Hh, G4 = C, B4 = Vv
    blue site   R4 = X,  G4 = P, B4 = C           green between blues in its row   R4 = Vv, G4 = C, B4 = Hh
    gray        (4899 R4 + 9617 G4 + 1868 B4 + 32768) >> 16

Everything is an integer.  `scale` composes this with tests/scale_model.py: the crop is a Bayer frame of its own (its phase shifted
by the crop's origin, neighbours mirrored at the crop's edges) and its gray plane is area-averaged.  `encode` goes the other way for
the stream tests: the mosaic a sensor behind that filter would record of a colourised gray frame."""
import numpy as np

from tests import scale_model as sm

RGGB8, GRBG8, GBRG8, BGGR8, RGGB16, GRBG16, GBRG16, BGGR16 = range(16, 24)
FORMATS = tuple(range(16, 24))
NAMES = {RGGB8: "bayer_rggb8", GRBG8: "bayer_grbg8", GBRG8: "bayer_gbrg8", BGGR8: "bayer_bggr8", RGGB16: "bayer_rggb16",
         GRBG16: "bayer_grbg16", GBRG16: "bayer_gbrg16", BGGR16: "bayer_bggr16"}
BYTES = {f: 1 if f < RGGB16 else 2 for f in FORMATS}
PHASE = {RGGB8: (0, 0), GRBG8: (1, 0), GBRG8: (0, 1), BGGR8: (1, 1), RGGB16: (0, 0), GRBG16: (1, 0), GBRG16: (0, 1), BGGR16: (1, 1)}


def samples(px, fmt, bits=0):
    """[..., h, w, BYTES[fmt]] uint8 -> the 8-bit samples [..., h, w] int64"""
    assert px.dtype == np.uint8 and px.shape[-1] == BYTES[fmt], (px.dtype, px.shape, fmt)
    p = px.astype(np.int64)
    if BYTES[fmt] == 1:
        return p[..., 0]
    b = bits or 16
    assert 8 <= b <= 16, bits
    return np.minimum(255, (p[..., 0] | (p[..., 1] << 8)) >> (b - 8))


def sites(h, w, phase):
    """-> boolean [h][w] masks: red, green between reds, green between blues, blue"""
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy = (xx + phase[0]) & 1, (yy + phase[1]) & 1
    return (cx == 0) & (cy == 0), (cx == 1) & (cy == 0), (cx == 0) & (cy == 1), (cx == 1) & (cy == 1)


def gray_of_samples(s, phase):
    """samples [..., h, w] (integers 0..255) of a mosaic with pattern phase (px, py) -> gray [..., h, w] uint8"""
    s = np.asarray(s).astype(np.int64)
    h, w = s.shape[-2:]
    assert h >= 2 and w >= 2
    p = np.pad(s, [(0, 0)] * (s.ndim - 2) + [(1, 1), (1, 1)], mode="reflect")
    left, right, up, down = p[..., 1:-1, :-2], p[..., 1:-1, 2:], p[..., :-2, 1:-1], p[..., 2:, 1:-1]
    C = 4 * s
    P = left + right + up + down
    X = p[..., :-2, :-2] + p[..., :-2, 2:] + p[..., 2:, :-2] + p[..., 2:, 2:]
    Hh, Vv = 2 * (left + right), 2 * (up + down)
    red, g_red, g_blue, blue = sites(h, w, phase)
    R4 = np.where(red, C, np.where(blue, X, np.where(g_red, Hh, Vv)))
    G4 = np.where(red | blue, P, C)
    B4 = np.where(blue, C, np.where(red, X, np.where(g_red, Vv, Hh)))
    g = (4899 * R4 + 9617 * G4 + 1868 * B4 + 32768) >> 16
    assert g.min(initial=0) >= 0 and g.max(initial=0) <= 255
    return g.astype(np.uint8)


def reduce(px, fmt, bits=0):
    """A mosaic [..., h, w, BYTES[fmt]] uint8 -> its gray plane [..., h, w] uint8"""
    return gray_of_samples(samples(px, fmt, bits), PHASE[fmt])


def scale(px, geo, W, H, fmt, bits=0):
    """A mosaic [..., src_height, src_width, BYTES[fmt]] larger than the W x H plane, geo = (src_width, src_height, crop_x, crop_y, cw,
    ch) -> [..., H, W] uint8: the crop demosaiced as a frame of its own, then the area mean of tests/scale_model.py"""
    sm.check(geo, W, H)
    sw, sh, x, y, cw, ch = geo
    assert px.shape[-3:-1] == (sh, sw), (px.shape, geo)
    phase = ((PHASE[fmt][0] + x) & 1, (PHASE[fmt][1] + y) & 1)
    g = gray_of_samples(samples(px[..., y:y + ch, x:x + cw, :], fmt, bits), phase)
    return sm.scale_gray(g, (cw, ch, 0, 0, cw, ch), W, H)


def encode(g, fmt, bits=0, seed=3):
    """gray [..., h, w] -> the mosaic [..., h, w, BYTES[fmt]] of the frame colourised as tests/pixfmt_model.py: encode does (B = g,
    G = min(255, g + g // 8), R = g - g // 4): every site holds its colour's value; *16: in the top 8 of `bits` bits, seeded noise below"""
    y = g.astype(np.int64)
    h, w = g.shape[-2:]
    red, g_red, g_blue, blue = sites(h, w, PHASE[fmt])
    v = np.where(red, y - y // 4, np.where(blue, y, np.minimum(255, y + y // 8)))
    if BYTES[fmt] == 1:
        return np.ascontiguousarray(v[..., None].astype(np.uint8))
    b = bits or 16
    v = (v << (b - 8)) | np.random.RandomState(seed).randint(0, 1 << (b - 8), size=g.shape)
    return np.ascontiguousarray(np.stack([v & 255, v >> 8], -1).astype(np.uint8))
