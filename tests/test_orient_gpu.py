"""Turned and mirrored frames at the inner plug point (include/xrslam_hip.h: xrhip_klt_set_orientation).

The turn is a kernel of its own behind the unchanged uploads (k_orient) and moves bytes: every comparison here is assert_array_equal
against tests/orient_model.py -- the gray crop turned by the formulas, then scaled by tests/scale_model.py -- through
xrhip_debug_get_raw.

Working planes (96,67), (97,66), (98,65), (99,64): every W % 4, aligned dwords of the plane that straddle a row end, H no multiple of
k_orient's 64-pixel tile and W a tile plus a part; (40,33): smaller than one tile in both dimensions; (65,65): one tile plus one
pixel in each.  An HBM source is an allocation that ENDS with the frame's last needed byte (tests/color_frames.py: Hbm)."""
import ctypes as C

import numpy as np
import pytest

from tests import bayer_model as bm
from tests import color_frames as cf
from tests import orient_model as om
from tests import pixfmt_model as pm
from tests import scale_model as sm
from tests.test_scale_gpu import frame, geometries, needed_bytes
from tests.util import noise_image

pytestmark = pytest.mark.gpu

PLANES = [(96, 67), (97, 66), (98, 65), (99, 64), (40, 33), (65, 65)]
PADS = (0, 5, 64)
ORIENTATIONS = tuple(range(8))
# one format per byte class: (format, bits, limited_range)
VARIANTS = [(pm.GRAY8, 0, 0), (pm.GRAY16, 10, 0), (pm.YUYV, 0, 0), (pm.RGB8, 0, 0), (pm.BGRA8, 0, 0)]
GEOMETRIES = ("ratio 1, crop offset", "coprime", "2x by 1x")


def _name(v):
    return "%s bits %d limited %d" % (pm.NAMES[v[0]], v[1], v[2])


def want_plane(gray, geo, o, W, H):
    """The definition: the gray crop of the source frame, turned, then scaled to the plane (geo None: the whole frame)"""
    if geo is not None:
        _, _, x, y, cw, ch = geo
        gray = gray[y:y + ch, x:x + cw]
    u = om.orient(gray, o)
    th, tw = u.shape
    return sm.scale_gray(u, (tw, th, 0, 0, tw, th), W, H)


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
        c.set_orientation(0)
        c.synchronize()


@pytest.fixture()
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


def _frame_bytes(view):
    """The flat bytes of a strided [h][w][c] frame from its first to its last needed byte"""
    h, w, c = view.shape
    return view.strides[0] * (h - 1) + w * c


@pytest.mark.parametrize("W,H", PLANES)
def test_oriented_gray_frames_equal_the_model(contexts, hbm, W, H):
    """8-bit gray, all eight orientations: host frames with row padding 0, 5 and 64, HBM frames at base offsets 0..3 whose allocation ends
    with the frame's last byte."""
    ctx = contexts(W, H)
    im = ctx.image()
    for o in ORIENTATIONS:
        ctx.set_orientation(o)
        assert ctx.get_orientation() == o
        fw, fh = om.turned_size(W, H, o)
        assert ctx.frame_size() == (fw, fh)
        for pad in PADS:
            g = noise_image(fw, fh, seed=100 + 8 * pad + o)
            flat, view = frame(g[:, :, None], pad)
            want = om.orient(g, o)
            assert want.shape == (H, W)
            im.upload_format(view, pm.GRAY8)
            np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, pad %d, host" % (o, pad))
            if pad == 0:
                im.upload(g)
                np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, xrhip_image_upload" % o)
            tail = flat[:_frame_bytes(view)]
            for off in (0, 1, 2, 3):
                im.upload_device(hbm.put(tail, off), view.strides[0])
                np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, pad %d, HBM at base offset %d" % (o, pad, off))
        hbm.close()
    ctx.set_orientation(0)


@pytest.mark.parametrize("W,H", [(97, 66), (98, 65)])
@pytest.mark.parametrize("v", VARIANTS, ids=[_name(v).replace(" ", "_") for v in VARIANTS])
def test_oriented_formats_and_geometries_equal_the_model(contexts, hbm, W, H, v):
    """One format per byte class, unscaled and through three geometries (ratio 1 with a crop offset, coprime, 2x by 1x) whose crop covers
    the TURNED plane; host and HBM sources."""
    fmt, bits, lim = v
    bpp = pm.BYTES[fmt]
    ctx = contexts(W, H)
    im = ctx.image()
    for o in ORIENTATIONS:
        ctx.set_orientation(o)
        fw, fh = om.turned_size(W, H, o)
        px = cf.random_pixels(fw, fh, bpp, seed=10 * fmt + o + W)
        flat, view = frame(px, 5)
        want = want_plane(pm.reduce(px, fmt, bits, lim), None, o, W, H)
        im.upload_format(view, fmt, bits, lim)
        np.testing.assert_array_equal(im.raw(), want, err_msg="%s, o %d, host" % (_name(v), o))
        im.upload_format(hbm.put(flat[:_frame_bytes(view)], o % 4), fmt, bits, lim, on_device=True, stride=view.strides[0])
        np.testing.assert_array_equal(im.raw(), want, err_msg="%s, o %d, HBM" % (_name(v), o))
        geos = geometries(fw, fh)
        for k, name in enumerate(GEOMETRIES):
            geo = geos[name]
            px = cf.random_pixels(geo[0], geo[1], bpp, seed=1000 * fmt + 10 * o + k + W)
            flat, view = frame(px, (0, 5, 64)[k])
            want = want_plane(pm.reduce(px, fmt, bits, lim), geo, o, W, H)
            im.upload_scaled(view, geo, fmt, bits, lim)
            np.testing.assert_array_equal(im.raw(), want, err_msg="%s, o %d, %s, host" % (_name(v), o, name))
            tail = flat[:needed_bytes(geo, bpp, view.strides[0])]
            im.upload_scaled(hbm.put(tail, (o + k) % 4), geo, fmt, bits, lim, on_device=True, stride=view.strides[0])
            np.testing.assert_array_equal(im.raw(), want, err_msg="%s, o %d, %s, HBM" % (_name(v), o, name))
        hbm.close()
    ctx.set_orientation(0)


@pytest.mark.parametrize("fmt,bits", [(bm.GRBG8, 0), (bm.BGGR16, 12)], ids=["bayer_grbg8", "bayer_bggr16_bits12"])
def test_oriented_bayer_mosaics_equal_the_model(contexts, hbm, fmt, bits):
    """A mosaic is demosaiced in source coordinates -- its phase, and the mirroring at the frame's or the crop's edges, mean what they
    meant -- and the gray plane is turned: unscaled, and scaled with an odd crop origin."""
    W, H = 97, 66
    bpp = bm.BYTES[fmt]
    ctx = contexts(W, H)
    im = ctx.image()
    for o in ORIENTATIONS:
        ctx.set_orientation(o)
        fw, fh = om.turned_size(W, H, o)
        px = cf.random_pixels(fw, fh, bpp, seed=300 + fmt + o)
        flat, view = frame(px, 5)
        want = om.orient(bm.reduce(px, fmt, bits), o)
        im.upload_format(view, fmt, bits)
        np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, host" % o)
        im.upload_format(hbm.put(flat[:_frame_bytes(view)], 1), fmt, bits, on_device=True, stride=view.strides[0])
        np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, HBM" % o)
        geo = geometries(fw, fh)["odd crop origin"]
        cw, ch = geo[4], geo[5]
        px = cf.random_pixels(geo[0], geo[1], bpp, seed=400 + fmt + o)
        flat, view = frame(px, 64)
        crop_gray = bm.scale(px, geo, cw, ch, fmt, bits)             # (ratio 1: the crop demosaiced as a frame of its own)
        want = want_plane(crop_gray, None, o, W, H)
        im.upload_scaled(view, geo, fmt, bits)
        np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, scaled, host" % o)
        tail = flat[:needed_bytes(geo, bpp, view.strides[0])]
        im.upload_scaled(hbm.put(tail, 3), geo, fmt, bits, on_device=True, stride=view.strides[0])
        np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, scaled, HBM" % o)
        hbm.close()
    ctx.set_orientation(0)


def test_oriented_distorted_uploads_equal_the_undistorted_model_plane(klt, hbm):
    """Turned first, rectified second: oracle/undistort.py applied to the model's working plane, through every distorted entry point --
    the gray HBM frame included, which orientation 0 alone remaps where it lies."""
    from oracle import undistort as ou
    from tests.test_color_gpu import UNDIST
    model, W, H, K, D = UNDIST[0]
    ctx = klt.KltContext(W, H, 150)
    ctx.set_undistort_map(ou.packed_map(W, H, K, D, model))
    im = ctx.image()

    def rectified(plane):
        want = ou.undistort_model(plane, K, D, model)
        assert (want != plane).mean() > 0.5                       # the lens model does move the pixels
        return want
    for o in (1, 6, 0):
        ctx.set_orientation(o)
        fw, fh = om.turned_size(W, H, o)
        g = noise_image(fw, fh, seed=60 + o)
        want = rectified(om.orient(g, o))
        im.upload_distorted(g)
        np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, host gray" % o)
        flat, view = frame(g[:, :, None], 5)
        im.upload_distorted_device(hbm.put(flat[:_frame_bytes(view)], 1), view.strides[0])
        np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, HBM gray" % o)
        rgb = pm.encode(g, pm.RGB8)
        want_rgb = rectified(om.orient(pm.reduce(rgb, pm.RGB8), o))
        im.upload_format_distorted(rgb, pm.RGB8)
        np.testing.assert_array_equal(im.raw(), want_rgb, err_msg="o %d, RGB8" % o)
        im.upload_color_distorted(hbm.put(rgb[..., ::-1].copy(), 2), on_device=True, stride=3 * fw, channels=3)
        np.testing.assert_array_equal(im.raw(), want_rgb, err_msg="o %d, BGR8 in HBM" % o)
        geo = (fw + 60, fh + 40, 7, 3, fw + 50, fh + 30)
        big = noise_image(geo[0], geo[1], seed=80 + o)
        im.upload_scaled_distorted(big, geo)
        np.testing.assert_array_equal(im.raw(), rectified(want_plane(big, geo, o, W, H)), err_msg="o %d, scaled" % o)
        hbm.close()
    ctx.synchronize()


def test_orientations_change_between_the_uploads_of_one_context(klt, hbm):
    """Orientation 0 after a non-zero one is the plain upload again; the setting can change between any two uploads."""
    W, H = 98, 65
    ctx = klt.KltContext(W, H, 50)
    im, other = ctx.image(), ctx.image()
    plain = noise_image(W, H, seed=5)
    for k, o in enumerate((3, 0, 6, 1, 1, 0, 5, 2, 7, 4, 0)):
        ctx.set_orientation(o)
        fw, fh = om.turned_size(W, H, o)
        g = noise_image(fw, fh, seed=20 + k)
        (im if k % 2 else other).upload(g)
        np.testing.assert_array_equal((im if k % 2 else other).raw(), om.orient(g, o), err_msg="step %d, o %d" % (k, o))
        if o == 0:
            im.upload(plain)
            np.testing.assert_array_equal(im.raw(), plain)
            im.upload_device(hbm.put(plain), W)
            np.testing.assert_array_equal(im.raw(), plain)
    ctx.synchronize()


def test_rejected_orientations_and_frames_leave_the_plane_and_the_setting(klt):
    from xrslam_amd import _lib
    W, H = 98, 65
    ctx = klt.KltContext(W, H, 50)
    im = ctx.image()
    L = klt.L()
    err = _lib.lib().xrhip_last_error
    ctx.set_orientation(3)
    before_src = noise_image(H, W, seed=2)
    im.upload(before_src)
    before = om.orient(before_src, 3)
    np.testing.assert_array_equal(im.raw(), before)
    for bad in (8, -1):
        assert L.xrhip_klt_set_orientation(ctx._h, bad) == _lib.XRHIP_EINVAL and b"orientation" in err()
        assert ctx.get_orientation() == 3
    assert L.xrhip_klt_set_orientation(None, 1) == _lib.XRHIP_EINVAL
    assert L.xrhip_klt_get_orientation(ctx._h, None) == _lib.XRHIP_EINVAL
    # the frame is H wide in memory: a stride below that row is refused (the plane's own width W would have been enough before)
    assert H < W
    g = noise_image(H, W, seed=3)
    p = g.ctypes.data_as(C.c_void_p)
    assert L.xrhip_image_upload(im._h, p, H - 1) == _lib.XRHIP_EINVAL and b"stride" in err()
    assert L.xrhip_image_upload_device(im._h, p, H - 1) == _lib.XRHIP_EINVAL and b"stride" in err()
    assert L.xrhip_image_upload_format(im._h, p, 2 * H - 1, pm.GRAY16, 0, 0, 0) == _lib.XRHIP_EINVAL and b"stride" in err()
    ctx.set_orientation(2)   # (even: the row is W)
    assert L.xrhip_image_upload(im._h, p, W - 1) == _lib.XRHIP_EINVAL and b"stride" in err()
    ctx.set_orientation(3)
    # a crop that covers W x H but not the turned H x W
    from xrslam_amd import abi
    big = cf.random_pixels(W + 10, W + 10, 1, seed=4)
    for geo in ((W + 10, W + 10, 0, 0, W, H), (W + 10, W + 10, 0, 0, W + 10, W - 1), (W + 10, W + 10, 0, 0, H - 1, W)):
        gg = abi.FrameGeometry(*geo)
        assert L.xrhip_image_upload_scaled(im._h, big.ctypes.data_as(C.c_void_p), W + 10, pm.GRAY8, 0, 0, 0, C.byref(gg)) == _lib.XRHIP_EINVAL, geo
        assert b"crop_" in err(), err()
    assert ctx.get_orientation() == 3
    np.testing.assert_array_equal(im.raw(), before)             # the earlier plane is still there, unchanged
    # the context still works
    geo = (W + 10, W + 10, 1, 2, H + 3, W + 1)
    im.upload_scaled(big, geo)
    np.testing.assert_array_equal(im.raw(), want_plane(big[:, :, 0], geo, 3, W, H))
    ctx.synchronize()


def test_a_group_member_turns_its_frames_behind_its_pending_upload(klt):
    """A context joined to an instance group defers its uploads; the turn is a launch of its own behind them.  Frames through four
    entry points and four orientations, more of them than there are pinned slots, none waited for; only then are the planes read."""
    from xrslam_amd import _lib
    lib = _lib.lib()
    lib.xrhip_group_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.xrhip_group_destroy.argtypes = [C.c_void_p]
    lib.xrhip_klt_join_group.argtypes = [C.c_void_p, C.c_void_p]
    W, H = 97, 66
    ctx = klt.KltContext(W, H, 50)
    ims = [ctx.image() for _ in range(5)]
    group = C.c_void_p()
    assert lib.xrhip_group_create(C.byref(group)) == 0
    assert lib.xrhip_klt_join_group(ctx._h, group) == 0, lib.xrhip_last_error()
    try:
        for rnd in range(2):
            want = []
            for k, o in enumerate((1, 0, 6, 7, 2)):
                ctx.set_orientation(o)
                fw, fh = om.turned_size(W, H, o)
                if k == 2:
                    px = cf.random_pixels(fw, fh, 4, seed=31 + rnd)
                    ims[k].upload_color(px)
                    want.append(om.orient(pm.reduce(px, pm.BGRA8), o))
                elif k == 3:
                    geo = geometries(fw, fh)["coprime"]
                    _, big = frame(cf.random_pixels(geo[0], geo[1], 3, seed=51 + rnd), 5)
                    ims[k].upload_scaled(big, geo, pm.RGB8)
                    want.append(want_plane(pm.reduce(big, pm.RGB8), geo, o, W, H))
                else:
                    g = noise_image(fw, fh, seed=11 + 10 * rnd + k)
                    ims[k].upload(g)
                    want.append(om.orient(g, o))
            for k, (im, w) in enumerate(zip(ims, want)):
                np.testing.assert_array_equal(im.raw(), w, err_msg="round %d, image %d" % (rnd, k))
        ctx.synchronize()
    finally:
        for im in ims:
            im.close()
        lib.xrhip_klt_join_group(ctx._h, None)
        ctx.close()
        lib.xrhip_group_destroy(group)
