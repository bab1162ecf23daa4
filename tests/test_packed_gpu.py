"""Packed 10 / 12-bit camera frames at the inner plug point (include/xrslam_hip.h: XRHIP_PIXFMT_GRAY*_MIPI, GRAY*P and their BAYER_*
forms through xrhip_image_upload_format, _scaled and their _distorted forms).

The unpacker is a device kernel of its own (k_upload_packed) and moves bits: every comparison here is assert_array_equal of
xrhip_debug_get_raw against tests/packed_model.py -- the existing GRAY16 / BAYER_*16 / scale / orient models over the unpacked samples.
HBM sources are allocated through the HIP runtime the library is linked to (tests/color_frames.py: Hbm) and end with the frame's
last needed byte.

Planes (96,67), (97,66), (98,65), (99,64): every w % 4, so from the second row on a lane's four pixels start at every bit phase of
the row's stream and at every position of a MIPI group, aligned dwords of the plane straddle row ends, and the plane's last
w * h % 4 pixels go one by one; more than one block.  752 x 480 once per format."""
import ctypes as C

import numpy as np
import pytest

from tests import color_frames as cf
from tests import orient_model as om
from tests import packed_model as pk

pytestmark = pytest.mark.gpu

PLANES = [(96, 67), (97, 66), (98, 65), (99, 64)]
PADS = (0, 5, 64)
IDS = [pk.NAMES[f] for f in pk.FORMATS]


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


def packed(w, h, fmt, seed):
    """Seeded random samples over the whole range of the format's bits, packed: dense rows [h][row bytes]"""
    return pk.pack(pk.random_samples(w, h, pk.PACKING[fmt], seed), pk.PACKING[fmt])


def tail(view, w, h, fmt, x0=0, y0=0):
    """The flat bytes of a (padded) packed frame from its first byte to the last byte that holds a needed sample"""
    n = pk.needed_bytes(w, h, view.strides[0], pk.PACKING[fmt], x0, y0)
    return np.lib.stride_tricks.as_strided(view, shape=(n,), strides=(1,))


@pytest.mark.parametrize("fmt", pk.FORMATS, ids=IDS)
def test_upload_format_packed_equals_the_model(contexts, hbm, fmt):
    """Rows padded by 0, 5 and 64 bytes; a host source, and HBM sources at base offsets 0..3; limited_range on the mono forms; a frame
    of extremes (samples 0 and 2^bits - 1) reaches gray 0 and 255."""
    mono = fmt in pk.MONO
    for w, h in PLANES:
        im = contexts(w, h).image()
        for pad in PADS:
            rows = pk.padded(packed(w, h, fmt, seed=1000 * fmt + 10 * pad + w), pad)
            for lim in ((0, 1) if mono else (0,)):
                want = pk.reduce(rows, w, fmt, lim)
                what = "%s %dx%d, row padding %d, limited %d" % (pk.NAMES[fmt], w, h, pad, lim)
                im.upload_format(rows, fmt, 0, lim)
                np.testing.assert_array_equal(im.raw(), want, err_msg=what + ", host")
                for off in (0, 1, 2, 3):
                    im.upload_format(hbm.put(tail(rows, w, h, fmt), off), fmt, 17, lim, on_device=True, stride=rows.strides[0])   # (`bits` is not read)
                    np.testing.assert_array_equal(im.raw(), want, err_msg="%s, HBM at base offset %d" % (what, off))
            hbm.close()
        top = (1 << pk.BITS[pk.PACKING[fmt]]) - 1
        ext = np.zeros((h, w), np.int64)
        ext[:, w // 2:] = top
        ext[h // 2:, :3] = top
        rows = pk.padded(pk.pack(ext, pk.PACKING[fmt]), 5)
        want = pk.reduce(rows, w, fmt)
        assert want.min() == 0 and want.max() == 255
        if mono:
            np.testing.assert_array_equal(want, np.where(ext > 0, 255, 0))
        im.upload_format(rows, fmt)
        np.testing.assert_array_equal(im.raw(), want, err_msg="extremes")


@pytest.mark.parametrize("fmt", pk.FORMATS, ids=IDS)
def test_upload_format_packed_at_the_sensor_size(klt, contexts, hbm, fmt):
    w, h = 752, 480
    im = contexts(w, h).image()
    rows = pk.padded(packed(w, h, fmt, seed=fmt), 5)
    want = pk.reduce(rows, w, fmt)
    im.upload_format(rows, fmt)
    np.testing.assert_array_equal(im.raw(), want, err_msg="host")
    im.upload_format(hbm.put(tail(rows, w, h, fmt), 1), fmt, on_device=True, stride=rows.strides[0])
    np.testing.assert_array_equal(im.raw(), want, err_msg="HBM")


def scaled_geometries(W, H):
    """(src_width, src_height, crop_x, crop_y, cw, ch): a 2W+1 x 2H+1 crop at odd origins (the crop starts mid-group, the Bayer phase
    shifts in both axes; non-integer ratio), the same at an even row and column 2 (mid-group for the 10-bit forms only), a ratio-1 crop"""
    return {"2w+1 x 2h+1 at (3, 5)": (2 * W + 6, 2 * H + 7, 3, 5, 2 * W + 1, 2 * H + 1),
            "2w+1 x 2h+1 at (2, 0)": (2 * W + 3, 2 * H + 1, 2, 0, 2 * W + 1, 2 * H + 1),
            "ratio 1 at (1, 1)": (W + 3, H + 2, 1, 1, W, H)}


@pytest.mark.parametrize("fmt", pk.FORMATS, ids=IDS)
def test_upload_scaled_packed_equals_the_model(contexts, hbm, fmt):
    """Only the byte groups that hold a crop pixel are read: the HBM source ends with the last of them."""
    mono = fmt in pk.MONO
    for W, H in ((33, 32), (34, 33)):
        im = contexts(W, H).image()
        for name, geo in scaled_geometries(W, H).items():
            rows = pk.padded(packed(geo[0], geo[1], fmt, seed=77 * fmt + geo[2] + W), 5)
            for lim in ((0, 1) if mono else (0,)):
                want = pk.scale(rows, geo, W, H, fmt, lim)
                what = "%s -> %dx%d, %s, limited %d" % (pk.NAMES[fmt], W, H, name, lim)
                im.upload_scaled(rows, geo, fmt, 0, lim)
                np.testing.assert_array_equal(im.raw(), want, err_msg=what + ", host")
                needed = tail(rows, geo[4], geo[5], fmt, geo[2], geo[3])
                for off in (0, 1, 3):
                    im.upload_scaled(hbm.put(needed, off), geo, fmt, 0, lim, on_device=True, stride=rows.strides[0])
                    np.testing.assert_array_equal(im.raw(), want, err_msg="%s, HBM at base offset %d" % (what, off))
            if name.startswith("ratio 1") and mono:
                s = pk.unpack(rows, geo[0], pk.PACKING[fmt])[1:1 + H, 1:1 + W]
                np.testing.assert_array_equal(pk.scale(rows, geo, W, H, fmt), s >> (pk.BITS[pk.PACKING[fmt]] - 8))
        hbm.close()


@pytest.mark.parametrize("fmt", [33, 34, 40, 55], ids=lambda f: pk.NAMES[f])
def test_oriented_packed_frames_equal_the_model(contexts, hbm, fmt):
    """Orientations 1 (a quarter turn), 2 (a half turn) and 5 (mirrored + a quarter turn): the frame is unpacked (and demosaiced) in the
    source's orientation, then turned; unscaled and scaled, host and HBM."""
    W, H = 97, 66
    ctx = contexts(W, H)
    im = ctx.image()
    try:
        for o in (1, 2, 5):
            ctx.set_orientation(o)
            fw, fh = om.turned_size(W, H, o)
            rows = pk.padded(packed(fw, fh, fmt, seed=fmt + o), 5)
            want = om.orient(pk.reduce(rows, fw, fmt), o)
            assert want.shape == (H, W)
            im.upload_format(rows, fmt)
            np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, host" % o)
            im.upload_format(hbm.put(tail(rows, fw, fh, fmt), 3), fmt, on_device=True, stride=rows.strides[0])
            np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, HBM" % o)
            geo = (2 * fw + 6, 2 * fh + 7, 3, 5, 2 * fw + 1, 2 * fh + 1)
            big = packed(geo[0], geo[1], fmt, seed=fmt + 10 * o)
            # (exact area scaling commutes with the orientations: the source-orientation plane is what is turned)
            want = om.orient(pk.scale(big, geo, fw, fh, fmt), o)
            im.upload_scaled(big, geo, fmt)
            np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, scaled, host" % o)
            im.upload_scaled(hbm.put(tail(big, geo[4], geo[5], fmt, geo[2], geo[3]), 1), geo, fmt, on_device=True, stride=big.strides[0])
            np.testing.assert_array_equal(im.raw(), want, err_msg="o %d, scaled, HBM" % o)
    finally:
        ctx.set_orientation(0)


def test_packed_distorted_is_unpacked_first_and_rectified_second(klt, hbm):
    from tests.test_bayer_gpu import remap_packed, synthetic_map
    w, h = 34, 33
    ctx = klt.KltContext(w, h, 50)
    im = ctx.image()
    rows = pk.padded(packed(w, h, 32, seed=1), 5)
    L, err = klt.L(), klt.L().xrhip_last_error
    p = rows.ctypes.data_as(C.c_void_p)
    from xrslam_amd import _lib
    assert L.xrhip_image_upload_format_distorted(im._h, p, rows.strides[0], 32, 0, 0, 0) == _lib.XRHIP_ESTATE and b"map" in err()
    m = synthetic_map(w, h)
    ctx.set_undistort_map(m)
    for fmt in (32, 35, 45, 50):
        rows = pk.padded(packed(w, h, fmt, seed=fmt), 5)
        plane = pk.reduce(rows, w, fmt)
        want = remap_packed(m, plane)
        assert (want != plane).mean() > 0.5
        im.upload_format_distorted(rows, fmt)
        np.testing.assert_array_equal(im.raw(), want, err_msg=pk.NAMES[fmt] + ", host")
        im.upload_format_distorted(hbm.put(tail(rows, w, h, fmt), 1), fmt, on_device=True, stride=rows.strides[0])
        np.testing.assert_array_equal(im.raw(), want, err_msg=pk.NAMES[fmt] + ", HBM")
        geo = (70, 67, 3, 5, 61, 59)
        big = packed(geo[0], geo[1], fmt, seed=fmt + 1)
        im.upload_scaled_distorted(big, geo, fmt)
        np.testing.assert_array_equal(im.raw(), remap_packed(m, pk.scale(big, geo, w, h, fmt)), err_msg=pk.NAMES[fmt] + ", scaled")
    ctx.synchronize()


@pytest.mark.parametrize("fmt", [32, 33, 34, 35, 43, 52], ids=lambda f: pk.NAMES[f])
def test_an_hbm_frame_of_exactly_its_size_between_two_guards(klt, hbm, fmt):
    """Three allocations in a row -- guard, the frame in exactly row_bytes * h bytes, guard -- at base offset 0: the plane is the
    model's and both guards still hold their pattern (the upload writes nothing outside its own buffers; reads of the frame stay
    inside the aligned dwords that hold its bytes)."""
    hip = hbm.hip
    for w, h in ((97, 66), (99, 64)):
        ctx = klt.KltContext(w, h, 50)
        im = ctx.image()
        rows = packed(w, h, fmt, seed=fmt + w)
        guard = np.full(4096, 0xC3, np.uint8)
        a = hbm.put(guard)
        src = hbm.put(rows)
        b = hbm.put(guard)
        im.upload_format(src, fmt, on_device=True, stride=rows.shape[1])
        np.testing.assert_array_equal(im.raw(), pk.reduce(rows, w, fmt))
        geo = (w, h, 1, 1, w - 1, h - 1)
        small = klt.KltContext(w // 2, h // 2, 50)
        sim = small.image()
        sim.upload_scaled(src, geo, fmt, on_device=True, stride=rows.shape[1])
        np.testing.assert_array_equal(sim.raw(), pk.scale(rows, geo, w // 2, h // 2, fmt))
        for g in (a, b):
            back = np.zeros_like(guard)
            assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), C.c_void_p(g), C.c_size_t(guard.size), 2) == 0
            np.testing.assert_array_equal(back, guard)
        small.synchronize()
        ctx.synchronize()
        hbm.close()


def test_packed_error_codes_leave_the_plane_and_the_context_intact(klt):
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
    plain = [lambda fmt, lim, stride, ptr=p, fn=fn: fn(im._h, ptr, stride, fmt, 0, lim, 0)
             for fn in (L.xrhip_image_upload_format, L.xrhip_image_upload_format_distorted)]
    scaled = [lambda fmt, lim, stride, ptr=p, fn=fn: fn(im._h, ptr, stride, fmt, 0, lim, 0, C.byref(geo))
              for fn in (L.xrhip_image_upload_scaled, L.xrhip_image_upload_scaled_distorted)]
    for calls, cols in ((plain, w), (scaled, 2 * w)):
        for call in calls:
            for fmt in (11, 15, 24, 25, 31, 36, 39, 56, 64):
                assert call(fmt, 0, 4 * cols) == _lib.XRHIP_EINVAL and b"format" in err(), fmt
            for fmt in pk.FORMATS:
                row = pk.row_bytes(cols, pk.PACKING[fmt])
                if fmt in pk.BAYER:
                    assert call(fmt, 1, row) == _lib.XRHIP_EINVAL and b"limited_range" in err(), pk.NAMES[fmt]
                assert call(fmt, 0, row - 1) == _lib.XRHIP_EINVAL and b"stride" in err(), pk.NAMES[fmt]
                assert call(fmt, 0, row, ptr=None) == _lib.XRHIP_EINVAL and b"pixels" in err(), pk.NAMES[fmt]
            np.testing.assert_array_equal(im.raw(), before)       # the earlier plane is still there, unchanged
    # and the context still works
    rows = packed(w, h, 47, seed=3)
    im.upload_format(rows, 47)
    np.testing.assert_array_equal(im.raw(), pk.reduce(rows, w, 47))


def test_a_group_member_unpacks_in_its_own_order_without_waiting(klt):
    """A context joined to an instance group defers its shared upload; the packed launches go out behind it on the group's queue.
    Gray, packed mono, scaled packed mosaic, packed mosaic and gray host frames, one per image, none read before all are queued."""
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
            m10, b12 = pk.padded(packed(W, H, 32, seed=31 + rnd), 5), packed(W, H, 54, seed=41 + rnd)
            big = packed(geo[0], geo[1], 41, seed=51 + rnd)
            ims[0].upload(g0)
            ims[1].upload_format(m10, 32, 0, 1)
            ims[2].upload_scaled(big, geo, 41)
            ims[3].upload_format(b12, 54)
            ims[4].upload(g1)
            want = [g0, pk.reduce(m10, W, 32, 1), pk.scale(big, geo, W, H, 41), pk.reduce(b12, W, 54), g1]
            for k, (im, w) in enumerate(zip(ims, want)):
                np.testing.assert_array_equal(im.raw(), w, err_msg="round %d, image %d" % (rnd, k))
        ctx.synchronize()
    finally:
        for im in ims:
            im.close()
        lib.xrhip_klt_join_group(ctx._h, None)
        ctx.close()
        lib.xrhip_group_destroy(group)
