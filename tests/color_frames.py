"""Colour frames for the colour-input tests, and the reference they are held to.

`gray_ref` is cv::cvtColor BGR(A)2GRAY in its 14-bit fixed point, gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14, in numpy
int32: what the host pipeline computed for channel 3 / 4 frames before the conversion moved into the device upload, and what the
CPU reference build still computes.  `colorize` builds a BGR / BGRA frame from a gray one as a function of the gray values alone
(B = g, G = min(255, g + g//8), R = g - g//4; alpha from a seeded generator): the texture moves with the scene, so a stream of such
frames tracks like the gray stream, and the three channels differ, so a swapped or dropped channel changes the result."""
import ctypes as C

import numpy as np


def gray_ref(px):
    """[..., h, w, 3 or 4] uint8 (byte 0 = B, 1 = G, 2 = R, 3 ignored) -> [..., h, w] uint8"""
    p = px.astype(np.int32)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def strided(px, pad, seed=7):
    """The same pixels in rows of w * channels + pad bytes (the padding holds seeded noise): a view, [..., h, w, c]."""
    if pad == 0:
        return np.ascontiguousarray(px)
    *lead, h, w, c = px.shape
    buf = np.random.RandomState(seed).randint(0, 256, size=(*lead, h, w * c + pad), dtype=np.uint8)
    buf[..., :w * c] = px.reshape(*lead, h, w * c)
    row = w * c + pad
    strides = tuple(buf.strides[:-2]) + (row, c, 1)
    out = np.lib.stride_tricks.as_strided(buf, shape=px.shape, strides=strides)
    assert np.array_equal(out, px)
    return out


def colorize(g, channels, pad=0, seed=11):
    """gray [..., h, w] -> BGR / BGRA [..., h, w, channels] (see the module docstring), rows padded by `pad` bytes"""
    g16 = g.astype(np.int32)
    planes = [g16, np.minimum(255, g16 + g16 // 8), g16 - g16 // 4]
    if channels == 4:
        planes.append(np.random.RandomState(seed).randint(0, 256, size=g.shape))
    return strided(np.stack(planes, -1).astype(np.uint8), pad)


def random_pixels(w, h, channels, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, channels), dtype=np.uint8)


def extreme_pixels(w, h, channels):
    """Every combination of 0 / 1 / 254 / 255 per channel, repeated over the frame"""
    v = np.array([0, 1, 254, 255], np.uint8)
    combos = np.stack(np.meshgrid(*([v] * channels), indexing="ij"), -1).reshape(-1, channels)
    idx = np.arange(w * h) % len(combos)
    return np.ascontiguousarray(combos[idx].reshape(h, w, channels))


class Hbm:
    """Device buffers through the HIP runtime the library itself is linked to (a second runtime in the process -- torch brings its
    own copy -- cannot be initialised after the first, and other tests of the session have started this one)."""

    def __init__(self):
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so.7")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipDeviceSynchronize.argtypes = []
        self.hip = hip
        self.bufs = []

    def put(self, arr, offset=0):
        """The bytes of `arr`'s buffer (rows with their padding) at `offset` bytes past an allocation's start -> device address"""
        nbytes = int(sum((n - 1) * st for n, st in zip(arr.shape, arr.strides)) + 1)   # first to last byte of the (strided) view
        dev = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(dev), C.c_size_t(nbytes + offset)) == 0
        self.bufs.append(dev)
        assert self.hip.hipMemcpy(C.c_void_p(dev.value + offset), C.c_void_p(arr.ctypes.data), C.c_size_t(nbytes), 1) == 0
        return dev.value + offset

    def close(self):
        self.hip.hipDeviceSynchronize()
        for d in self.bufs:
            assert self.hip.hipFree(d) == 0
        self.bufs = []
