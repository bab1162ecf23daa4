"""The camera pixel formats in plain numpy: the yardstick of the pixel-format tests.

A frame is a uint8 array [..., h, w, bytes per pixel] (for NV12 / I420 / P010: the luma plane; rows may be strided).  `reduce`
gives the 8-bit gray plane the tracker works on, per pixel, all in integers:

    GRAY8, NV12, I420   the byte
    BGR8, BGRA8         (B*1868 + G*9617 + R*4899 + 8192) >> 14          byte 3 ignored
    RGB8, RGBA8         (R*4899 + G*9617 + B*1868 + 8192) >> 14          byte 3 ignored
    GRAY16              v = b0 | b1 << 8; bits in 8..16, 0 means 16;  min(255, v >> (bits - 8))
    YUYV / UYVY         byte 0 / byte 1 of the pixel's pair
    P010                the high byte of the 16-bit sample
    limited_range       afterwards: min(255, ((max(gray, 16) - 16) * 255 + 109) // 219); not for the four RGB / BGR formats

`encode` goes the other way for the stream tests: a frame of the format whose bytes are a function of a gray frame (plus seeded
noise in the bits and bytes that must be ignored), so that a stream of such frames tracks like the gray stream."""
import numpy as np

GRAY8, BGR8, BGRA8, RGB8, RGBA8, GRAY16, YUYV, UYVY, NV12, I420, P010 = range(11)
NAMES = ("gray8", "bgr8", "bgra8", "rgb8", "rgba8", "gray16", "yuyv", "uyvy", "nv12", "i420", "p010")
BYTES = {GRAY8: 1, BGR8: 3, BGRA8: 4, RGB8: 3, RGBA8: 4, GRAY16: 2, YUYV: 2, UYVY: 2, NV12: 1, I420: 1, P010: 2}
NO_RANGE_FLAG = (BGR8, BGRA8, RGB8, RGBA8)


def expand_limited(g):
    g = np.asarray(g).astype(np.int64)
    return np.minimum(255, ((np.maximum(g, 16) - 16) * 255 + 109) // 219)


def reduce(px, fmt, bits=0, limited_range=0):
    """[..., h, w, BYTES[fmt]] uint8 -> [..., h, w] uint8"""
    assert px.dtype == np.uint8 and px.shape[-1] == BYTES[fmt], (px.dtype, px.shape, fmt)
    p = px.astype(np.int64)
    if fmt in (GRAY8, NV12, I420, YUYV):
        g = p[..., 0]
    elif fmt in (UYVY, P010):
        g = p[..., 1]
    elif fmt in (BGR8, BGRA8):
        g = (p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14
    elif fmt in (RGB8, RGBA8):
        g = (p[..., 0] * 4899 + p[..., 1] * 9617 + p[..., 2] * 1868 + 8192) >> 14
    elif fmt == GRAY16:
        b = bits or 16
        assert 8 <= b <= 16, bits
        g = np.minimum(255, (p[..., 0] | (p[..., 1] << 8)) >> (b - 8))
    else:
        raise ValueError(fmt)
    if limited_range:
        assert fmt not in NO_RANGE_FLAG
        g = expand_limited(g)
    return g.astype(np.uint8)


def samples16(v):
    """16-bit samples [...] -> little-endian bytes [..., 2]"""
    v = np.asarray(v).astype(np.int64)
    return np.stack([v & 255, v >> 8], -1).astype(np.uint8)


def encode(g, fmt, bits=0, limited_range=0, seed=3):
    """gray [..., h, w] -> a frame [..., h, w, BYTES[fmt]] of the format (see the module docstring)"""
    rs = np.random.RandomState(seed)
    y = g.astype(np.int64)
    if limited_range:   # video levels 16..235
        y = 16 + (y * 219 + 127) // 255
    if fmt in (GRAY8, NV12, I420):
        out = y[..., None]
    elif fmt in (YUYV, UYVY):
        c = rs.randint(0, 256, size=g.shape)
        out = np.stack([y, c] if fmt == YUYV else [c, y], -1)
    elif fmt == GRAY16:
        b = bits or 16
        out = samples16((y << (b - 8)) | rs.randint(0, 1 << (b - 8), size=g.shape))
    elif fmt == P010:   # 10 significant bits at the top of the sample, the low 6 are zero
        out = samples16(((y << 2) | rs.randint(0, 4, size=g.shape)) << 6)
    else:
        planes = [y, np.minimum(255, y + y // 8), y - y // 4]   # B, G, R as tests/color_frames.py: colorize
        if fmt in (RGB8, RGBA8):
            planes = planes[::-1]
        if BYTES[fmt] == 4:
            planes.append(rs.randint(0, 256, size=g.shape))
        out = np.stack(planes, -1)
    return np.ascontiguousarray(out.astype(np.uint8))
