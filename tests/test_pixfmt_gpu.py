"""Camera pixel formats at the inner plug point (include/xrslam_hip.h: xrhip_image_upload_format, _format_distorted).

The reduction to gray is part of the device upload (k_upload) and is integer arithmetic: every comparison here is
assert_array_equal against tests/pixfmt_model.py.  HBM sources are allocated through the HIP runtime the library is linked to
(tests/color_frames.py: Hbm says why not through torch).

Shapes: (96,67), (97,66), (98,65), (99,64) -- every w % 4, groups of four pixels that straddle a row end, a plane whose last
w*h % 4 pixels go byte by byte -- and one (752,480).  A frame in HBM always ends at the end of its allocation (Hbm.put allocates
first byte to last byte of the strided view, plus the base offset): the upload needs nothing behind the frame's last row."""
import ctypes as C

import numpy as np
import pytest

from tests import color_frames as cf
from tests import pixfmt_model as pm
from tests.util import noise_image

pytestmark = pytest.mark.gpu

SHAPES = [(96, 67), (97, 66), (98, 65), (99, 64), (752, 480)]
PADS = (0, 5, 64)
# (format, bits, limited_range): every new format, with and without the range flag where it is allowed
VARIANTS = ([(pm.RGB8, 0, 0), (pm.RGBA8, 0, 0), (pm.GRAY8, 0, 1)]
            + [(pm.GRAY16, b, lim) for b in (8, 10, 12, 16) for lim in (0, 1)]
            + [(f, 0, lim) for f in (pm.YUYV, pm.UYVY, pm.NV12, pm.I420, pm.P010) for lim in (0, 1)])
GROUPS = {"rgb": [v for v in VARIANTS if v[0] in (pm.RGB8, pm.RGBA8)], "gray16": [v for v in VARIANTS if v[0] == pm.GRAY16],
          "packed": [v for v in VARIANTS if v[0] in (pm.YUYV, pm.UYVY)],
          "planar": [v for v in VARIANTS if v[0] in (pm.NV12, pm.I420, pm.P010, pm.GRAY8)]}


def _name(v):
    return "%s bits %d limited %d" % (pm.NAMES[v[0]], v[1], v[2])


@pytest.fixture(scope="module")
def klt():
    from xrslam_amd import klt
    return klt


@pytest.fixture(scope="module")
def contexts(klt):
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = klt.KltContext(w, h, 50)
        return made[(w, h)]
    yield get
    for c in made.values():
        c.synchronize()


@pytest.fixture()
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


def _extremes(w, h, fmt, bits):
    if fmt == pm.GRAY16:   # 0, 2^bits - 1, 2^bits, 65535 (2^16 does not fit: 65535 twice)
        b = bits or 16
        v = np.array([0, (1 << b) - 1, min(1 << b, 65535), 65535])
        return pm.samples16(v[np.arange(w * h) % 4].reshape(h, w))
    return cf.extreme_pixels(w, h, pm.BYTES[fmt])


def _check_sources(im, hbm, px, want, v, what, offsets=(0, 1, 2, 3)):
    fmt, bits, lim = v
    im.upload_format(px, fmt, bits, lim)
    np.testing.assert_array_equal(im.raw(), want, err_msg="%s, %s, host" % (_name(v), what))
    for off in offsets:
        im.upload_format(hbm.put(px, off), fmt, bits, lim, on_device=True, stride=px.strides[0])
        np.testing.assert_array_equal(im.raw(), want, err_msg="%s, %s, HBM at base offset %d" % (_name(v), what, off))


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_upload_format_equals_the_model(contexts, hbm, w, h, group):
    """Seeded random bytes and an extremes frame; row padding 0, 5, 64; host source, and HBM source at base offsets 0..3 (1 and 3:
    misaligned 16-bit samples).  The extremes frame reaches both ends of the gray range."""
    im = contexts(w, h).image()
    for v in GROUPS[group]:
        fmt, bits, lim = v
        for pad in PADS:
            px = cf.strided(cf.random_pixels(w, h, pm.BYTES[fmt], seed=1000 * fmt + 10 * bits + pad + w), pad)
            _check_sources(im, hbm, px, pm.reduce(px, fmt, bits, lim), v, "random, row padding %d" % pad)
        px = cf.strided(_extremes(w, h, fmt, bits), 5)
        want = pm.reduce(px, fmt, bits, lim)
        assert want.min() == 0 and want.max() == 255, _name(v)
        _check_sources(im, hbm, px, want, v, "extremes", offsets=(0, 3))
        hbm.close()


def _guarded(hbm, raw):
    """`raw` (1-d bytes) in an allocation of exactly its size, between two guard allocations -> (address, check)"""
    guard = np.full(4096, 0xA5, np.uint8)
    before = hbm.put(guard)
    dev = hbm.put(raw)
    after = hbm.put(guard)

    def check():
        for g in (before, after):
            back = np.zeros_like(guard)
            assert hbm.hip.hipMemcpy(C.c_void_p(back.ctypes.data), C.c_void_p(g), C.c_size_t(back.nbytes), 2) == 0
            np.testing.assert_array_equal(back, guard)
    return dev, check


@pytest.mark.parametrize("w,h", SHAPES[:4])
def test_upload_format_needs_nothing_beyond_the_frame(contexts, hbm, w, h):
    """NV12 / I420 / P010: the HBM source is exactly stride * height bytes, the luma plane alone.  The packed formats: exactly
    stride * (height - 1) + width * bytes per pixel.  The frame ends where its allocation ends; the result is the model's and the
    neighbouring allocations keep their bytes."""
    im = contexts(w, h).image()
    for fmt in (pm.NV12, pm.I420, pm.P010, pm.YUYV, pm.UYVY, pm.GRAY16, pm.RGB8):
        bpp = pm.BYTES[fmt]
        planar = fmt in (pm.NV12, pm.I420, pm.P010)
        for pad in (0, 5):
            stride = w * bpp + pad
            n = stride * h if planar else stride * (h - 1) + w * bpp
            raw = np.random.RandomState(fmt * 10 + pad).randint(0, 256, size=n, dtype=np.uint8)
            rows = np.zeros(stride * h, np.uint8)
            rows[:n] = raw
            px = rows.reshape(h, stride)[:, :w * bpp].reshape(h, w, bpp)
            dev, check = _guarded(hbm, raw)
            im.upload_format(dev, fmt, 0, 0, on_device=True, stride=stride)
            np.testing.assert_array_equal(im.raw(), pm.reduce(px, fmt), err_msg="%s, row padding %d" % (pm.NAMES[fmt], pad))
            check()
        hbm.close()


@pytest.mark.parametrize("v", [(pm.YUYV, 0, 0), (pm.RGB8, 0, 0)], ids=["yuyv", "rgb8"])
def test_preprocess_after_upload_format_equals_preprocess_of_the_gray_frame(klt, v):
    w, h = 752, 480
    fmt, bits, lim = v
    ctx = klt.KltContext(w, h, 150)
    px = cf.strided(pm.encode(noise_image(w, h, seed=9 + fmt), fmt, bits, lim), 5)
    a, b = ctx.image(), ctx.image(pm.reduce(px, fmt, bits, lim))
    a.upload_format(px, fmt, bits, lim)
    a.preprocess()
    b.preprocess()
    for l in range(4):
        (ia, da), (ib, db) = a.level(l), b.level(l)
        np.testing.assert_array_equal(ia, ib, err_msg="level %d image" % l)
        np.testing.assert_array_equal(da, db, err_msg="level %d derivatives" % l)


def test_upload_format_distorted_equals_upload_distorted_of_the_gray_frame(klt, hbm):
    """Reduced to gray first, rectified second: the same bits as the model's gray frame through xrhip_image_upload_distorted."""
    from oracle import undistort as ou
    from tests.test_color_gpu import UNDIST
    model, w, h, K, D = UNDIST[0]
    assert model == "radtan"
    ctx = klt.KltContext(w, h, 150)
    ctx.set_undistort_map(ou.packed_map(w, h, K, D, model))
    fmt, bits, lim = pm.GRAY16, 10, 1
    px = cf.strided(pm.encode(noise_image(w, h, seed=41), fmt, bits, lim), 64)
    g = pm.reduce(px, fmt, bits, lim)
    ref = ctx.image()
    ref.upload_distorted(g)
    want = ref.raw()
    assert (want != g).mean() > 0.5                       # the lens model does move the pixels
    im = ctx.image()
    im.upload_format_distorted(px, fmt, bits, lim)
    np.testing.assert_array_equal(im.raw(), want)
    im.upload_format_distorted(hbm.put(px, 1), fmt, bits, lim, on_device=True, stride=px.strides[0])
    np.testing.assert_array_equal(im.raw(), want)
    ctx.synchronize()


def test_upload_format_error_codes_and_the_context_survives(klt):
    from xrslam_amd import _lib
    w, h = 98, 65
    ctx = klt.KltContext(w, h, 50)
    im = ctx.image()
    px = cf.random_pixels(w, h, 4, seed=1)
    p = px.ctypes.data_as(klt.C.c_void_p)
    L = klt.L()
    err = _lib.lib().xrhip_last_error
    for fn in (L.xrhip_image_upload_format, L.xrhip_image_upload_format_distorted):
        for fmt in (-1, 11, 99):
            assert fn(im._h, p, w * 4, fmt, 0, 0, 0) == _lib.XRHIP_EINVAL
            assert b"format" in err()
        for bits in (7, 17):
            assert fn(im._h, p, w * 2, pm.GRAY16, bits, 0, 0) == _lib.XRHIP_EINVAL
            assert b"bits" in err()
        for fmt in (pm.GRAY16, pm.YUYV, pm.RGB8, pm.RGBA8, pm.NV12, pm.P010):
            assert fn(im._h, p, w * pm.BYTES[fmt] - 1, fmt, 0, 0, 0) == _lib.XRHIP_EINVAL   # short stride
            assert b"stride" in err()
        for fmt in pm.NO_RANGE_FLAG:
            assert fn(im._h, p, w * 4, fmt, 0, 1, 0) == _lib.XRHIP_EINVAL
            assert b"limited_range" in err()
        assert fn(im._h, None, w * 2, pm.YUYV, 0, 0, 0) == _lib.XRHIP_EINVAL
    assert L.xrhip_image_upload_format_distorted(im._h, p, w * 2, pm.YUYV, 0, 0, 0) == _lib.XRHIP_ESTATE   # no undistortion map
    assert b"map" in err()
    # the context still uploads correctly
    yuyv = np.ascontiguousarray(px[..., :2])
    im.upload_format(yuyv, pm.YUYV)
    np.testing.assert_array_equal(im.raw(), pm.reduce(yuyv, pm.YUYV))


def test_gray_bgr_and_new_formats_alternate_through_the_same_pinned_slots(klt):
    """Host frames of different sizes in turn: the slots grow with the first wide frame and every later frame still arrives whole.
    GRAY8, BGR8 and BGRA8 through xrhip_image_upload_format are the frames of the older entry points."""
    w, h = 97, 66
    ctx = klt.KltContext(w, h, 50)
    im = ctx.image()
    g = noise_image(w, h, seed=3)
    for rnd in range(2):
        im.upload(g)
        np.testing.assert_array_equal(im.raw(), g)
        for k, v in enumerate([(pm.GRAY16, 12, 0), (pm.BGR8, 0, 0), (pm.UYVY, 0, 1), (pm.GRAY8, 0, 0), (pm.RGBA8, 0, 0), (pm.NV12, 0, 1),
                               (pm.BGRA8, 0, 0), (pm.P010, 0, 0)]):
            fmt, bits, lim = v
            px = cf.strided(cf.random_pixels(w, h, pm.BYTES[fmt], seed=50 + 10 * rnd + k), 5 * (k % 2))
            im.upload_format(px, fmt, bits, lim)
            np.testing.assert_array_equal(im.raw(), pm.reduce(px, fmt, bits, lim), err_msg=_name(v))
            if fmt in (pm.BGR8, pm.BGRA8):
                np.testing.assert_array_equal(im.raw(), cf.gray_ref(px))
        im.upload(g[::-1].copy())
        np.testing.assert_array_equal(im.raw(), g[::-1])
    ctx.synchronize()
