"""Bayer raw mosaics at the inner plug point (include/xrslam_hip.h: XRHIP_PIXFMT_BAYER_* through xrhip_image_upload_format, _scaled
and their _distorted forms).

The demosaic is a device kernel of its own (k_upload_bayer) and integer arithmetic: every comparison here is assert_array_equal of
xrhip_debug_get_raw against tests/bayer_model.py.  HBM sources are allocated through the HIP runtime the library is linked to
(tests/color_frames.py: Hbm) and end with the frame's last needed byte.

Planes 32, 33, 34, 35 x 33: every w % 4 -- groups of four pixels that straddle a row end, a plane whose last w*h % 4 pixels go one by
one -- an odd height, more than one block (35 * 33 / 4 > 256 lanes), and first / last rows and columns (the mirrored neighbours) are
a large share of so small a plane."""
import ctypes as C

import numpy as np
import pytest

from tests import bayer_model as bm
from tests import color_frames as cf
from tests import pixfmt_model as pm
from tests.test_scale_gpu import frame, needed_bytes

pytestmark = pytest.mark.gpu

WIDTHS = (32, 33, 34, 35)
HEIGHT = 33
IDS = [bm.NAMES[f] for f in bm.FORMATS]
# (src_width, src_height, crop_x, crop_y, cw, ch) -> 32 x 32
SCALED = {"odd crop origin, non-integer ratio": (70, 67, 3, 5, 61, 59), "2x": (64, 64, 0, 0, 64, 64), "plain crop at (1, 0)": (40, 36, 1, 0, 32, 32)}


def bits_of(fmt):
    return (10, 12, 0) if bm.BYTES[fmt] == 2 else (0,)


def mosaic(w, h, fmt, bits, seed):
    """Seeded random samples, mostly inside the significant bits (a few above: they saturate)"""
    rs = np.random.RandomState(seed)
    px = rs.randint(0, 256, size=(h, w, bm.BYTES[fmt]), dtype=np.uint8)
    if bm.BYTES[fmt] == 2 and bits:
        over = rs.randint(0, 16, size=(h, w)) == 0
        px[..., 1] = np.where(over, px[..., 1], px[..., 1] & ((1 << (bits - 8)) - 1))
    return px


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


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("fmt", bm.FORMATS, ids=IDS)
def test_upload_format_bayer_equals_the_model(contexts, hbm, w, fmt):
    """Dense rows and rows padded by 5 bytes; a host source, and HBM sources at base offsets 0, 1 and 3 (16-bit samples at odd
    addresses); bits 10, 12 and 0 for the 16-bit formats; a frame of extremes reaches both ends of the gray range."""
    h = HEIGHT
    im = contexts(w, h).image()
    for bits in bits_of(fmt):
        for pad in (0, 5):
            px = cf.strided(mosaic(w, h, fmt, bits, seed=1000 * fmt + 10 * bits + pad + w), pad)
            want = bm.reduce(px, fmt, bits)
            what = "%s, bits %d, row padding %d" % (bm.NAMES[fmt], bits, pad)
            im.upload_format(px, fmt, bits)
            np.testing.assert_array_equal(im.raw(), want, err_msg=what + ", host")
            for off in (0, 1, 3):
                im.upload_format(hbm.put(px, off), fmt, bits, on_device=True, stride=px.strides[0])
                np.testing.assert_array_equal(im.raw(), want, err_msg="%s, HBM at base offset %d" % (what, off))
        hbm.close()
    ext = np.zeros((h, w, bm.BYTES[fmt]), np.uint8)
    ext[:, w // 2:] = 255
    ext[h // 2:, :3] = 255
    want = bm.reduce(ext, fmt)
    assert want.min() == 0 and want.max() == 255 and len(np.unique(want)) > 4
    im.upload_format(cf.strided(ext, 5), fmt)
    np.testing.assert_array_equal(im.raw(), want, err_msg="extremes")


@pytest.mark.parametrize("name", sorted(SCALED))
@pytest.mark.parametrize("fmt", bm.FORMATS, ids=IDS)
def test_upload_scaled_bayer_equals_the_model(contexts, hbm, fmt, name):
    """The crop is a Bayer frame of its own: an odd crop origin shifts the pattern phase, neighbours mirror at the crop's edges, and
    the HBM source ends with the crop's last byte."""
    W = H = 32
    geo = SCALED[name]
    im = contexts(W, H).image()
    for bits in bits_of(fmt):
        px = mosaic(geo[0], geo[1], fmt, bits, seed=77 * fmt + bits + geo[2])
        want = bm.scale(px, geo, W, H, fmt, bits)
        flat, view = frame(px, 5)
        im.upload_scaled(view, geo, fmt, bits)
        np.testing.assert_array_equal(im.raw(), want, err_msg="%s, bits %d, host" % (name, bits))
        tail = flat[:needed_bytes(geo, bm.BYTES[fmt], view.strides[0])]
        for off in (0, 1):
            im.upload_scaled(hbm.put(tail, off), geo, fmt, bits, on_device=True, stride=view.strides[0])
            np.testing.assert_array_equal(im.raw(), want, err_msg="%s, bits %d, HBM at base offset %d" % (name, bits, off))
    if name.startswith("plain"):
        np.testing.assert_array_equal(want, bm.gray_of_samples(bm.samples(px[0:32, 1:33], fmt, bits), ((bm.PHASE[fmt][0] + 1) & 1, bm.PHASE[fmt][1])))


def test_a_crop_of_more_pixels_than_one_pass_of_the_grid(klt, hbm):
    """2048 x 1100 samples: more than the 2048 blocks x 1024 pixels the demosaic launch covers in one pass, so lanes take a second
    group of four; a host source (which also grows the slots and both scratches) and an HBM source, and a smaller frame afterwards."""
    W = H = 64
    geo = (2050, 1101, 1, 1, 2048, 1100)
    ctx = klt.KltContext(W, H, 50)
    im = ctx.image()
    px = mosaic(geo[0], geo[1], bm.GBRG8, 0, seed=4)
    want = bm.scale(px, geo, W, H, bm.GBRG8)
    assert want.std() > 1
    im.upload_scaled(px, geo, bm.GBRG8)
    np.testing.assert_array_equal(im.raw(), want, err_msg="host")
    im.upload_scaled(hbm.put(px.reshape(-1)[:needed_bytes(geo, 1, geo[0])]), geo, bm.GBRG8, on_device=True, stride=geo[0])
    np.testing.assert_array_equal(im.raw(), want, err_msg="HBM")
    small = mosaic(W, H, bm.BGGR16, 12, seed=5)
    im.upload_format(small, bm.BGGR16, 12)
    np.testing.assert_array_equal(im.raw(), bm.reduce(small, bm.BGGR16, 12))
    ctx.synchronize()


def remap_packed(map2, gray):
    """The packed 1/32-pixel inverse map of include/xrslam_hip.h applied to a gray plane: cv::remap(INTER_LINEAR, BORDER_CONSTANT 0)"""
    from oracle import undistort as ou
    sx = (map2[..., 0] & 0xffff).astype(np.uint16).view(np.int16).astype(np.int64)
    sy = (map2[..., 0] >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
    ax, ay = (map2[..., 1] & 255).astype(np.int64), ((map2[..., 1] >> 8) & 255).astype(np.int64)
    return ou._remap_fixed(gray, sx * 32 + ax, sy * 32 + ay)


def synthetic_map(w, h):
    """A small shear with sub-pixel offsets; some taps fall outside the plane (they read 0)"""
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    iu = 32 * x + (3 * x + 5 * y) % 97 - 40
    iv = 32 * y + (7 * x + y) % 61 - 20
    out = np.empty((h, w, 2), np.uint32)
    out[..., 0] = ((iu >> 5) & 0xffff).astype(np.uint32) | (((iv >> 5) & 0xffff).astype(np.uint32) << 16)
    out[..., 1] = (iu & 31).astype(np.uint32) | ((iv & 31).astype(np.uint32) << 8)
    return out


def test_bayer_distorted_is_demosaiced_first_and_rectified_second(klt, hbm):
    """Equal to remap_packed of the model's plane, unscaled and scaled, host and HBM.  The same calls with GRAY8 (limited range: the
    shared upload launch; plain: the remap of the frame where it lies) still give what tests/pixfmt_model.py says: the older path is
    as it was."""
    w, h = 34, 33
    ctx = klt.KltContext(w, h, 50)
    m = synthetic_map(w, h)
    ctx.set_undistort_map(m)
    im = ctx.image()
    for fmt, bits in ((bm.GRBG8, 0), (bm.BGGR16, 10)):
        px = cf.strided(mosaic(w, h, fmt, bits, seed=fmt), 5)
        plane = bm.reduce(px, fmt, bits)
        want = remap_packed(m, plane)
        assert (want != plane).mean() > 0.5
        im.upload_format_distorted(px, fmt, bits)
        np.testing.assert_array_equal(im.raw(), want, err_msg=bm.NAMES[fmt] + ", host")
        im.upload_format_distorted(hbm.put(px, 1), fmt, bits, on_device=True, stride=px.strides[0])
        np.testing.assert_array_equal(im.raw(), want, err_msg=bm.NAMES[fmt] + ", HBM")
        geo = (70, 67, 3, 5, 61, 59)
        big = mosaic(geo[0], geo[1], fmt, bits, seed=fmt + 1)
        im.upload_scaled_distorted(big, geo, fmt, bits)
        np.testing.assert_array_equal(im.raw(), remap_packed(m, bm.scale(big, geo, w, h, fmt, bits)), err_msg=bm.NAMES[fmt] + ", scaled")
    g = cf.strided(cf.random_pixels(w, h, 1, seed=9), 5)
    for lim in (0, 1):
        want = remap_packed(m, pm.reduce(g, pm.GRAY8, 0, lim))
        im.upload_format_distorted(g, pm.GRAY8, 0, lim)
        np.testing.assert_array_equal(im.raw(), want, err_msg="gray8, limited %d, host" % lim)
        im.upload_format_distorted(hbm.put(g, 1), pm.GRAY8, 0, lim, on_device=True, stride=g.strides[0])
        np.testing.assert_array_equal(im.raw(), want, err_msg="gray8, limited %d, HBM" % lim)
    ctx.synchronize()


def test_bayer_error_codes_leave_the_plane_and_the_context_intact(klt):
    from xrslam_amd import _lib, abi
    w, h = 34, 33
    ctx = klt.KltContext(w, h, 50)
    im = ctx.image()
    before = cf.random_pixels(w, h, 1, seed=2)[..., 0]
    im.upload(before)
    px = cf.random_pixels(2 * w, 2 * h, 2, seed=1)
    p = px.ctypes.data_as(C.c_void_p)
    L = klt.L()
    err = _lib.lib().xrhip_last_error
    geo = abi.FrameGeometry(2 * w, 2 * h, 1, 1, 2 * w - 1, 2 * h - 1)
    plain = [lambda fmt, bits, lim, stride, fn=fn: fn(im._h, p, stride, fmt, bits, lim, 0)
             for fn in (L.xrhip_image_upload_format, L.xrhip_image_upload_format_distorted)]
    scaled = [lambda fmt, bits, lim, stride, fn=fn: fn(im._h, p, stride, fmt, bits, lim, 0, C.byref(geo))
              for fn in (L.xrhip_image_upload_scaled, L.xrhip_image_upload_scaled_distorted)]
    for calls, cols in ((plain, w), (scaled, 2 * w)):
        for call in calls:
            for fmt in (11, 12, 13, 14, 15, 24):
                assert call(fmt, 0, 0, cols * 2) == _lib.XRHIP_EINVAL and b"format" in err(), fmt
            for fmt in bm.FORMATS:
                bpp = bm.BYTES[fmt]
                assert call(fmt, 0, 1, cols * bpp) == _lib.XRHIP_EINVAL and b"limited_range" in err(), bm.NAMES[fmt]
                assert call(fmt, 0, 0, cols * bpp - 1) == _lib.XRHIP_EINVAL and b"stride" in err(), bm.NAMES[fmt]
                for bits in (7, 17):
                    if bpp == 2:
                        assert call(fmt, bits, 0, cols * bpp) == _lib.XRHIP_EINVAL and b"bits" in err(), bm.NAMES[fmt]
            np.testing.assert_array_equal(im.raw(), before)       # the earlier plane is still there, unchanged
    assert L.xrhip_image_upload_format_distorted(im._h, p, w, bm.RGGB8, 0, 0, 0) == _lib.XRHIP_ESTATE and b"map" in err()   # no undistortion map
    np.testing.assert_array_equal(im.raw(), before)
    # `bits` is not read for the 8-bit formats, and the context still works
    one = mosaic(w, h, bm.RGGB8, 0, seed=3)
    im.upload_format(one, bm.RGGB8, 17)
    np.testing.assert_array_equal(im.raw(), bm.reduce(one, bm.RGGB8))


def test_a_group_member_demosaics_in_its_own_order_without_waiting(klt):
    """A context joined to an instance group defers its shared upload; the Bayer launch goes out behind it on the group's queue.
    Gray, Bayer, scaled Bayer and gray host frames, one per image, none read before all are queued: every plane is its model."""
    from xrslam_amd import _lib
    lib = _lib.lib()
    lib.xrhip_group_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.xrhip_group_destroy.argtypes = [C.c_void_p]
    lib.xrhip_klt_join_group.argtypes = [C.c_void_p, C.c_void_p]
    W, H = 35, 33
    geo = (2 * W + 6, 2 * H + 4, 3, 1, 2 * W + 1, 2 * H + 1)
    ctx = klt.KltContext(W, H, 50)
    ims = [ctx.image() for _ in range(5)]
    group = C.c_void_p()
    assert lib.xrhip_group_create(C.byref(group)) == 0
    assert lib.xrhip_klt_join_group(ctx._h, group) == 0, lib.xrhip_last_error()
    try:
        for rnd in range(2):
            g0, g1 = cf.random_pixels(W, H, 1, seed=11 + rnd)[..., 0], cf.random_pixels(W, H, 1, seed=21 + rnd)[..., 0]
            m8, m16 = mosaic(W, H, bm.GRBG8, 0, seed=31 + rnd), cf.strided(mosaic(W, H, bm.GBRG16, 12, seed=41 + rnd), 5)
            big = mosaic(geo[0], geo[1], bm.BGGR8, 0, seed=51 + rnd)
            ims[0].upload(g0)
            ims[1].upload_format(m8, bm.GRBG8)
            ims[2].upload_scaled(big, geo, bm.BGGR8)
            ims[3].upload_format(m16, bm.GBRG16, 12)
            ims[4].upload(g1)
            want = [g0, bm.reduce(m8, bm.GRBG8), bm.scale(big, geo, W, H, bm.BGGR8), bm.reduce(m16, bm.GBRG16, 12), g1]
            for k, (im, w) in enumerate(zip(ims, want)):
                np.testing.assert_array_equal(im.raw(), w, err_msg="round %d, image %d" % (rnd, k))
        ctx.synchronize()
    finally:
        for im in ims:
            im.close()
        lib.xrhip_klt_join_group(ctx._h, None)
        ctx.close()
        lib.xrhip_group_destroy(group)
