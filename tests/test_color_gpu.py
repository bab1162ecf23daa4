"""Colour frames at the inner plug point (include/xrslam_hip.h: xrhip_image_upload_color, xrhip_image_upload_color_distorted).

The reduction to gray is part of the device upload (k_upload, bytes per pixel 3 / 4) and is integer arithmetic: every comparison
here is assert_array_equal against tests/color_frames.py: gray_ref, the host pipeline's formula in numpy.  HBM sources are
allocated through the HIP runtime the library is linked to (color_frames.Hbm says why not through torch)."""
import numpy as np
import pytest

from tests import color_frames as cf
from tests.util import noise_image

pytestmark = pytest.mark.gpu

SIZES = [(752, 480), (641, 479), (352, 353), (1280, 720)]
PADS = (0, 5, 64)


@pytest.fixture(scope="module")
def klt():
    from xrslam_amd import klt
    return klt


@pytest.fixture()
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("channels", [3, 4])
def test_upload_color_equals_the_host_formula(klt, hbm, w, h, channels):
    """Seeded random bytes per channel; strides w*c, w*c + 5, w*c + 64; host source, and HBM source at base offsets 0..3."""
    ctx = klt.KltContext(w, h, 150)
    im = ctx.image()
    for pad in PADS:
        px = cf.strided(cf.random_pixels(w, h, channels, seed=100 * channels + pad + w), pad)
        want = cf.gray_ref(px)
        im.upload_color(px)
        np.testing.assert_array_equal(im.raw(), want, err_msg="host, stride w*c + %d" % pad)
        for off in (0, 1, 2, 3):
            dev = hbm.put(px, off)
            im.upload_color(dev, on_device=True, stride=px.strides[0], channels=channels)
            np.testing.assert_array_equal(im.raw(), want, err_msg="HBM, stride w*c + %d, base offset %d" % (pad, off))
    ctx.synchronize()


@pytest.mark.parametrize("channels", [3, 4])
def test_upload_color_extreme_values(klt, hbm, channels):
    """Every combination of 0 / 1 / 254 / 255 per channel (rounding at both ends of the 14-bit fixed point; 255 stays 255)."""
    w, h = 96, 67
    ctx = klt.KltContext(w, h, 50)
    px = cf.extreme_pixels(w, h, channels)
    want = cf.gray_ref(px)
    assert want.max() == 255 and want.min() == 0
    im = ctx.image()
    im.upload_color(px)
    np.testing.assert_array_equal(im.raw(), want)
    for off in (0, 3):
        im.upload_color(hbm.put(px, off), on_device=True, stride=px.strides[0], channels=channels)
        np.testing.assert_array_equal(im.raw(), want)
    ctx.synchronize()


@pytest.mark.parametrize("w,h", [(752, 480), (641, 479)])
@pytest.mark.parametrize("channels", [3, 4])
def test_preprocess_after_upload_color_equals_preprocess_of_the_gray_frame(klt, w, h, channels):
    ctx = klt.KltContext(w, h, 150)
    px = cf.colorize(noise_image(w, h, seed=5 + channels), channels, pad=5)
    a, b = ctx.image(), ctx.image(cf.gray_ref(px))
    a.upload_color(px)
    a.preprocess()
    b.preprocess()
    for l in range(4):
        (ia, da), (ib, db) = a.level(l), b.level(l)
        np.testing.assert_array_equal(ia, ib, err_msg="level %d image" % l)
        np.testing.assert_array_equal(da, db, err_msg="level %d derivatives" % l)


UNDIST = [("radtan", 752, 480, (458.654, 457.296, 367.215, 248.375), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)),
          ("equidistant", 512, 512, (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504),
           (0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182))]


@pytest.mark.parametrize("model,w,h,K,D", UNDIST, ids=[u[0] for u in UNDIST])
@pytest.mark.parametrize("channels", [3, 4])
def test_upload_color_distorted_equals_upload_distorted_of_the_gray_frame(klt, hbm, model, w, h, K, D, channels):
    """Reduced to gray first, rectified second: the same bits as the gray frame through xrhip_image_upload_distorted."""
    from oracle import undistort as ou
    ctx = klt.KltContext(w, h, 150)
    ctx.set_undistort_map(ou.packed_map(w, h, K, D, model))
    px = cf.colorize(noise_image(w, h, seed=31 + w), channels, pad=64)
    g = cf.gray_ref(px)
    ref = ctx.image()
    ref.upload_distorted(g)
    want = ref.raw()
    assert (want != g).mean() > 0.5                       # the lens model does move the pixels
    im = ctx.image()
    im.upload_color_distorted(px)
    np.testing.assert_array_equal(im.raw(), want)
    im.upload_color_distorted(hbm.put(px, 1), on_device=True, stride=px.strides[0], channels=channels)
    np.testing.assert_array_equal(im.raw(), want)
    ctx.synchronize()


def test_upload_color_error_codes_and_the_context_survives(klt):
    from xrslam_amd import _lib
    w, h = 352, 353
    ctx = klt.KltContext(w, h, 50)
    im = ctx.image()
    px = cf.random_pixels(w, h, 3, seed=1)
    L = klt.L()

    def rc_of(fn, ptr, stride, channels):
        return fn(im._h, ptr, stride, channels, 0)

    p = px.ctypes.data_as(klt.C.c_void_p)
    for fn in (L.xrhip_image_upload_color, L.xrhip_image_upload_color_distorted):
        for channels in (0, 2, 5, -1):
            assert rc_of(fn, p, w * 4, channels) == _lib.XRHIP_EINVAL
            assert b"channels" in _lib.lib().xrhip_last_error()
        assert rc_of(fn, None, w * 3, 3) == _lib.XRHIP_EINVAL
        assert rc_of(fn, p, w * 3 - 1, 3) == _lib.XRHIP_EINVAL          # short stride
        assert b"stride" in _lib.lib().xrhip_last_error()
        assert rc_of(fn, p, w * 4 - 1, 4) == _lib.XRHIP_EINVAL
    assert rc_of(L.xrhip_image_upload_color_distorted, p, w * 3, 3) == _lib.XRHIP_ESTATE   # no undistortion map
    assert b"map" in _lib.lib().xrhip_last_error()
    # the context still works afterwards
    im.upload_color(px)
    np.testing.assert_array_equal(im.raw(), cf.gray_ref(px))
    # channels 1 forwards to the gray upload
    g = cf.gray_ref(px)
    assert L.xrhip_image_upload_color(im._h, g.ctypes.data_as(klt.C.c_void_p), w, 1, 0) == 0
    np.testing.assert_array_equal(im.raw(), g)
    # gray after colour and colour after gray through the same (grown) pinned slots
    im.upload(g[::-1].copy())
    np.testing.assert_array_equal(im.raw(), g[::-1])
    px4 = cf.random_pixels(w, h, 4, seed=2)
    im.upload_color(px4)
    np.testing.assert_array_equal(im.raw(), cf.gray_ref(px4))
