"""Frames larger than the working plane at the inner plug point (include/xrslam_hip.h: xrhip_image_upload_scaled, _scaled_distorted).

The crop and the area mean are part of the device upload (k_upload_scaled) and are integer arithmetic: every comparison here is
assert_array_equal against tests/scale_model.py, through xrhip_debug_get_raw.

Working planes (96,67), (97,66), (98,65), (99,64): every W % 4, groups of four plane pixels that straddle a row end, a plane whose
last W*H % 4 pixels go one by one.  Geometries per plane: ratio 1 with a crop offset, exactly 2x, 3/2, a coprime non-integer ratio
(131 -> 97, 101 -> 66), a ratio above 8 (a footprint spans 9+ source pixels and rows), anisotropic (2x by 1x), odd crop_x / crop_y.
An HBM source is an allocation that ENDS with the crop's last needed byte (tests/color_frames.py: Hbm.put allocates first byte to
last byte of what it is given): the upload needs nothing behind it."""
import ctypes as C

import numpy as np
import pytest

from tests import color_frames as cf
from tests import pixfmt_model as pm
from tests import scale_model as sm
from tests.util import noise_image

pytestmark = pytest.mark.gpu

PLANES = [(96, 67), (97, 66), (98, 65), (99, 64)]
PADS = (0, 5, 64)
# one format per byte class and flag route: (format, bits, limited_range)
VARIANTS = [(pm.GRAY8, 0, 0), (pm.GRAY8, 0, 1), (pm.GRAY16, 10, 0), (pm.YUYV, 0, 0), (pm.UYVY, 0, 0), (pm.P010, 0, 1), (pm.RGB8, 0, 0),
            (pm.BGRA8, 0, 0)]


def _name(v):
    return "%s bits %d limited %d" % (pm.NAMES[v[0]], v[1], v[2])


def geometries(W, H):
    """name -> (src_width, src_height, crop_x, crop_y, cw, ch)"""
    return {"ratio 1, crop offset": (W + 9, H + 6, 5, 3, W, H),
            "2x": (2 * W, 2 * H, 0, 0, 2 * W, 2 * H),
            "3/2": ((3 * W + 1) // 2 + 2, (3 * H + 1) // 2, 2, 0, (3 * W + 1) // 2, (3 * H + 1) // 2),
            "coprime": (W + 40, H + 36, 6, 1, W + 34, H + 35),
            "above 8x": (8 * W + 4, 8 * H + 1, 1, 0, 8 * W + 3, 8 * H + 1),
            "2x by 1x": (2 * W + 1, H + 1, 0, 1, 2 * W, H),
            "odd crop origin": (W + W // 3 + 8, H + H // 5 + 8, 3, 5, W + W // 3, H + H // 5)}


def frame(px, pad, seed=7):
    """[h][w][bpp] pixels -> (the frame's bytes as one flat array, rows of w * bpp + pad bytes; the [h][w][bpp] view into it)"""
    h, w, c = px.shape
    row = w * c + pad
    buf = np.random.RandomState(seed).randint(0, 256, size=(h, row), dtype=np.uint8)
    buf[:, :w * c] = px.reshape(h, w * c)
    view = np.lib.stride_tricks.as_strided(buf, shape=px.shape, strides=(row, c, 1))
    return buf.reshape(-1), view


def needed_bytes(geo, bpp, stride):
    """bytes from the source frame's row 0 to the crop's last needed byte"""
    _, _, x, y, cw, ch = geo
    return stride * (y + ch - 1) + (x + cw) * bpp


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


def _check_sources(im, hbm, px, pad, geo, want, v, what, offsets):
    fmt, bits, lim = v
    flat, view = frame(px, pad)
    stride = view.strides[0]
    im.upload_scaled(view, geo, fmt, bits, lim)
    np.testing.assert_array_equal(im.raw(), want, err_msg="%s, %s, host" % (_name(v), what))
    tail = flat[:needed_bytes(geo, pm.BYTES[fmt], stride)]
    for off in offsets:
        im.upload_scaled(hbm.put(tail, off), geo, fmt, bits, lim, on_device=True, stride=stride)
        np.testing.assert_array_equal(im.raw(), want, err_msg="%s, %s, HBM at base offset %d" % (_name(v), what, off))


@pytest.mark.parametrize("W,H", PLANES)
@pytest.mark.parametrize("v", VARIANTS, ids=[_name(v).replace(" ", "_") for v in VARIANTS])
def test_upload_scaled_equals_the_model(contexts, hbm, W, H, v):
    """Seeded random bytes with row padding 0, 5, 64 and an extremes frame; a host source, and HBM sources at base offsets 0..3 that
    end with the crop's last byte."""
    from tests.test_pixfmt_gpu import _extremes
    fmt, bits, lim = v
    bpp = pm.BYTES[fmt]
    im = contexts(W, H).image()
    for k, (name, geo) in enumerate(geometries(W, H).items()):
        sw, sh = geo[:2]
        for pad in PADS:
            px = cf.random_pixels(sw, sh, bpp, seed=1000 * fmt + 10 * bits + pad + W + k)
            _check_sources(im, hbm, px, pad, geo, sm.scale(px, geo, W, H, fmt, bits, lim), v, "%s, random, row padding %d" % (name, pad), (0, 1, 2, 3))
        px = _extremes(sw, sh, fmt, bits)
        want = sm.scale(px, geo, W, H, fmt, bits, lim)
        if geo[4] == W and geo[5] == H:
            assert want.min() == 0 and want.max() == 255, _name(v)
        _check_sources(im, hbm, px, 5, geo, want, v, "%s, extremes" % name, (0, 3))
        hbm.close()


def test_1080p_nv12_luma_to_752x480(klt, hbm):
    """A decoder's 1920x1080 NV12 surface, 16:9 -> the tracker's 752x480 through the crop {114, 0, 1692, 1080}: only the luma rows of
    the crop are read (the HBM source ends with them)."""
    W, H = 752, 480
    geo = (1920, 1080, 114, 0, 1692, 1080)
    ctx = klt.KltContext(W, H, 150)
    im = ctx.image()
    surface = np.random.RandomState(12).randint(0, 256, size=(1080 + 540, 1920, 1), dtype=np.uint8)
    surface[:1080, :, 0] = noise_image(1920, 1080, seed=13)
    luma = surface[:1080]
    want = sm.scale(luma, geo, W, H, pm.NV12)
    assert want.std() > 20
    im.upload_scaled(surface[:1080], geo, pm.NV12)
    np.testing.assert_array_equal(im.raw(), want, err_msg="host")
    flat = surface.reshape(-1)[:needed_bytes(geo, 1, 1920)]
    for off in (0, 1):
        im.upload_scaled(hbm.put(flat, off), geo, pm.NV12, on_device=True, stride=1920)
        np.testing.assert_array_equal(im.raw(), want, err_msg="HBM at base offset %d" % off)
    want_lim = sm.scale(luma, geo, W, H, pm.NV12, 0, 1)
    im.upload_scaled(hbm.put(flat), geo, pm.NV12, 0, 1, on_device=True, stride=1920)
    np.testing.assert_array_equal(im.raw(), want_lim, err_msg="limited range")
    ctx.synchronize()


def test_the_largest_crop_stays_inside_32_bits(klt, hbm):
    """cw * ch = 2^24 exactly, every pixel 255: 255 * 2^24 + 2^23 is the largest sum there is, and the mean is 255 everywhere.  With one
    zero pixel in every 64 x 64 footprint, and with a zero block in every other one, the plane is what the model says."""
    W = H = 64
    n = 4096
    geo = (n, n, 0, 0, n, n)
    ctx = klt.KltContext(W, H, 50)
    im = ctx.image()
    g = np.full((n, n), 255, np.uint8)
    dev = hbm.put(g)
    im.upload_scaled(g, geo)
    np.testing.assert_array_equal(im.raw(), np.full((H, W), 255, np.uint8), err_msg="host")
    im.upload_scaled(dev, geo, on_device=True, stride=n)
    np.testing.assert_array_equal(im.raw(), np.full((H, W), 255, np.uint8), err_msg="HBM")
    hbm.close()
    g[32::64, 17::64] = 0
    g[64:128, 64:128][8:48, 8:48] = 0
    for by in range(0, n, 128):
        g[by + 3:by + 60, 5:50] = 0
    want = sm.scale_gray(g, geo, W, H)
    assert want[0, 1] == (255 * 4095 + 2048) // 4096 and len(np.unique(want)) >= 3
    im.upload_scaled(g, geo)
    np.testing.assert_array_equal(im.raw(), want, err_msg="host")
    im.upload_scaled(hbm.put(g), geo, on_device=True, stride=n)
    np.testing.assert_array_equal(im.raw(), want, err_msg="HBM")
    ctx.synchronize()


def test_upload_scaled_distorted_equals_upload_distorted_of_the_models_plane(klt, hbm):
    """Scaled first, rectified second: the same bits as the model's working plane through xrhip_image_upload_distorted; without a
    map the call is a state error."""
    from oracle import undistort as ou
    from tests.test_color_gpu import UNDIST
    from xrslam_amd import _lib
    model, W, H, K, D = UNDIST[0]
    ctx = klt.KltContext(W, H, 150)
    fmt, bits, lim = pm.GRAY16, 10, 1
    geo = (W + 200, H + 100, 7, 3, W + 150, H + 90)
    px = pm.encode(noise_image(geo[0], geo[1], seed=41), fmt, bits, lim)
    flat, view = frame(px, 64)
    im = ctx.image()
    g = FrameGeometry(klt, geo)
    assert klt.L().xrhip_image_upload_scaled_distorted(im._h, view.ctypes.data_as(C.c_void_p), view.strides[0], fmt, bits, lim, 0,
                                                       C.byref(g)) == _lib.XRHIP_ESTATE
    assert b"map" in _lib.lib().xrhip_last_error()
    ctx.set_undistort_map(ou.packed_map(W, H, K, D, model))
    plane = sm.scale(view, geo, W, H, fmt, bits, lim)
    ref = ctx.image()
    ref.upload_distorted(plane)
    want = ref.raw()
    assert (want != plane).mean() > 0.5                       # the lens model does move the pixels
    im.upload_scaled_distorted(view, geo, fmt, bits, lim)
    np.testing.assert_array_equal(im.raw(), want)
    tail = flat[:needed_bytes(geo, 2, view.strides[0])]
    im.upload_scaled_distorted(hbm.put(tail, 1), geo, fmt, bits, lim, on_device=True, stride=view.strides[0])
    np.testing.assert_array_equal(im.raw(), want)
    ctx.synchronize()


def FrameGeometry(klt, geo):
    from xrslam_amd import abi
    return abi.FrameGeometry(*geo)


def test_upload_scaled_error_codes_leave_the_plane_and_the_context_intact(klt):
    from xrslam_amd import _lib
    W, H = 98, 65
    ctx = klt.KltContext(W, H, 50)
    im = ctx.image()
    before = noise_image(W, H, seed=2)
    im.upload(before)
    sw, sh = 2 * W + 7, 2 * H + 5
    px = cf.random_pixels(sw, sh, 4, seed=1)
    p = px.ctypes.data_as(C.c_void_p)
    L = klt.L()
    err = _lib.lib().xrhip_last_error
    good = (sw, sh, 3, 1, 2 * W, 2 * H)

    def call(fn, geo, pixels=p, stride=sw * 4, fmt=pm.BGRA8, bits=0, lim=0, img=im._h):
        g = FrameGeometry(klt, geo) if geo is not None else None
        return fn(img, pixels, stride, fmt, bits, lim, 0, C.byref(g) if g is not None else None)

    for fn in (L.xrhip_image_upload_scaled, L.xrhip_image_upload_scaled_distorted):
        assert call(fn, good, pixels=None) == _lib.XRHIP_EINVAL and b"pixels" in err()
        assert call(fn, good, img=None) == _lib.XRHIP_EINVAL and b"img" in err()
        assert call(fn, None) == _lib.XRHIP_EINVAL and b"geo" in err()
        for geo in ((sw, sh, 8, 1, 2 * W, 2 * H), (sw, sh, 3, 6, 2 * W, 2 * H), (sw, sh, -1, 0, 2 * W, 2 * H), (sw, sh, 0, -1, 2 * W, 2 * H),
                    (sw, sh, 0, 0, sw + 1, sh), (sw, sh, 0, 0, sw, sh + 1), (sw, sh, 0, 0, 0, sh), (0, 0, 0, 0, 0, 0)):
            assert call(fn, geo) == _lib.XRHIP_EINVAL, geo
            assert b"crop" in err() or b"src_" in err(), err()
        assert call(fn, (sw, sh, 0, 0, W - 1, sh)) == _lib.XRHIP_EINVAL and b"crop_width" in err()      # no upscaling
        assert call(fn, (sw, sh, 0, 0, sw, H - 1)) == _lib.XRHIP_EINVAL and b"crop_height" in err()
        assert call(fn, (4097, 4096, 0, 0, 4097, 4096), stride=4097 * 4) == _lib.XRHIP_EINVAL and b"2^24" in err()
        assert call(fn, good, stride=sw * 4 - 1) == _lib.XRHIP_EINVAL and b"stride" in err()
        assert call(fn, good, fmt=99) == _lib.XRHIP_EINVAL and b"format" in err()
        assert call(fn, good, fmt=pm.GRAY16, bits=17) == _lib.XRHIP_EINVAL and b"bits" in err()
        assert call(fn, good, lim=1) == _lib.XRHIP_EINVAL and b"limited_range" in err()
        np.testing.assert_array_equal(im.raw(), before)       # the earlier plane is still there, unchanged
    assert call(L.xrhip_image_upload_scaled_distorted, good) == _lib.XRHIP_ESTATE and b"map" in err()
    np.testing.assert_array_equal(im.raw(), before)
    # the context still works
    im.upload_scaled(px, good, pm.BGRA8)
    np.testing.assert_array_equal(im.raw(), sm.scale(px, good, W, H, pm.BGRA8))


def test_plain_and_scaled_frames_alternate_through_the_same_context(klt, hbm):
    """Host frames of different sizes in turn share the pinned slots (which grow with the first large frame); every frame, plain
    or scaled, arrives whole."""
    W, H = 97, 66
    ctx = klt.KltContext(W, H, 50)
    im = ctx.image()
    g = noise_image(W, H, seed=3)
    geos = list(geometries(W, H).values())
    for rnd in range(2):
        for k, v in enumerate([(pm.GRAY8, 0, 0), (pm.YUYV, 0, 0), (pm.BGRA8, 0, 0), (pm.GRAY16, 12, 1), (pm.RGB8, 0, 0)]):
            fmt, bits, lim = v
            im.upload(g)
            np.testing.assert_array_equal(im.raw(), g)
            geo = geos[(k + 3 * rnd) % len(geos)]
            _, view = frame(cf.random_pixels(geo[0], geo[1], pm.BYTES[fmt], seed=50 + 10 * rnd + k), 5 * (k % 2))
            im.upload_scaled(view, geo, fmt, bits, lim)
            np.testing.assert_array_equal(im.raw(), sm.scale(view, geo, W, H, fmt, bits, lim), err_msg=_name(v))
            plain = cf.random_pixels(W, H, pm.BYTES[fmt], seed=70 + k)
            im.upload_format(plain, fmt, bits, lim)
            np.testing.assert_array_equal(im.raw(), pm.reduce(plain, fmt, bits, lim), err_msg=_name(v))
            flat, view = frame(cf.random_pixels(geo[0], geo[1], pm.BYTES[fmt], seed=90 + k), 5)
            dev = hbm.put(flat[:needed_bytes(geo, pm.BYTES[fmt], view.strides[0])], k % 4)
            im.upload_scaled(dev, geo, fmt, bits, lim, on_device=True, stride=view.strides[0])
            np.testing.assert_array_equal(im.raw(), sm.scale(view, geo, W, H, fmt, bits, lim), err_msg=_name(v))
        im.upload(g[::-1].copy())
        np.testing.assert_array_equal(im.raw(), g[::-1])
    ctx.synchronize()


def test_a_group_member_uploads_through_every_entry_point_without_waiting(klt):
    """A context joined to an instance group defers its uploads and never waits between them: five host frames, one per image and
    each through another entry point, more of them than there are pinned slots, the fourth a crop larger than anything staged before
    (the slots and the scaled upload's scratch grow while earlier uploads are in flight).  Only then are the planes read: every one
    is its model, bit for bit -- and again in a second round, with every buffer at its final size."""
    from xrslam_amd import _lib
    lib = _lib.lib()
    lib.xrhip_group_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.xrhip_group_destroy.argtypes = [C.c_void_p]
    lib.xrhip_klt_join_group.argtypes = [C.c_void_p, C.c_void_p]
    W, H = 97, 66
    geo = (2 * W + 6, 2 * H + 4, 3, 1, 2 * W + 1, 2 * H + 1)
    assert geo[4] * geo[5] * 3 > W * H * 4
    ctx = klt.KltContext(W, H, 50)
    ims = [ctx.image() for _ in range(5)]
    group = C.c_void_p()
    assert lib.xrhip_group_create(C.byref(group)) == 0
    assert lib.xrhip_klt_join_group(ctx._h, group) == 0, lib.xrhip_last_error()
    try:
        for rnd in range(2):
            g0, g1 = noise_image(W, H, seed=11 + rnd), noise_image(W, H, seed=21 + rnd)
            bgra = cf.random_pixels(W, H, 4, seed=31 + rnd)
            odd = np.zeros(1 + H * W * 2, np.uint8)
            yuyv = odd[1:].reshape(H, W, 2)                                   # (its first byte lies at an odd address)
            yuyv[...] = cf.random_pixels(W, H, 2, seed=41 + rnd)
            assert yuyv.ctypes.data % 2 == 1
            _, big = frame(cf.random_pixels(geo[0], geo[1], 3, seed=51 + rnd), 5)
            ims[0].upload(g0)
            ims[1].upload_color(bgra)
            ims[2].upload_format(yuyv, pm.YUYV)
            ims[3].upload_scaled(big, geo, pm.RGB8)
            ims[4].upload(g1)
            want = [g0, pm.reduce(bgra, pm.BGRA8), pm.reduce(yuyv, pm.YUYV), sm.scale(big, geo, W, H, pm.RGB8), g1]
            for k, (im, w) in enumerate(zip(ims, want)):
                np.testing.assert_array_equal(im.raw(), w, err_msg="round %d, image %d" % (rnd, k))
        ctx.synchronize()
    finally:
        for im in ims:
            im.close()
        lib.xrhip_klt_join_group(ctx._h, None)
        ctx.close()
        lib.xrhip_group_destroy(group)

