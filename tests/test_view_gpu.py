"""The tracking view at the inner plug point (include/xrslam_hip.h: xrhip_image_render_view) against tests/view_model.py.

Everything is integer: every comparison is assert_array_equal.  The primitives are seeded and carry the cases the renderer can get
wrong by construction (see _primitives); the model's answer is computed once per size and shared."""
import functools

import numpy as np
import pytest

from tests import color_frames as cf
from tests import view_model as vm
from tests.util import noise_image
from tests.view_hbm import HbmOut

pytestmark = pytest.mark.gpu

SIZES = [(67, 41), (96, 67), (352, 353), (752, 480)]   # widths 4k + 3, 4k, 4k (odd height), the workload's
PALETTE = [(0, 255, 255), (0, 0, 255), (0, 255, 0), (255, 255, 0), (255, 160, 0), (7, 8, 9), (250, 1, 128)]
POISON = 0xA5


@pytest.fixture(scope="module")
def klt():
    from xrslam_amd import klt
    return klt


@pytest.fixture()
def hbm():
    h = HbmOut()
    yield h
    h.close()


def _primitives(w, h, seed=5):
    """200 markers (x, y, palette, r2) and 400 segments (x0, y0, x1, y1, palette)"""
    r = np.random.RandomState(seed + w)
    np_ = len(PALETTE)
    mk = []
    for (x, y) in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)]:
        mk.append((x, y, len(mk) % np_, 10))                       # corners and edges
    for d in range(1, 13):                                         # 1 .. 12 pixels outside, on every side
        mk += [(-d, h // 3, d % np_, 10), (w - 1 + d, h // 2, d % np_, 10), (w // 3, -d, d % np_, 10), (w // 2, h - 1 + d, d % np_, 2)]
    mk += [(8191, 8191, 0, 10), (-8191, -8191, 1, 10), (8191, -8191, 2, 2), (-8191, 5, 3, 10), (5, 8191, 4, 10), (-8192, -8192, 5, 10)]
    sx, sy = w // 2 + 3, h // 2 - 2
    mk += [(sx, sy, k % np_, 10) for k in range(7)]                # a stack on one pixel, different palette entries
    mk += [(sx + 1, sy, 5, 2), (sx, sy + 1, 6, 0), (sx - 2, sy, 1, 25), (3, 3, 2, 100)]
    while len(mk) < 200:
        mk.append((int(r.randint(-8, w + 8)), int(r.randint(-8, h + 8)), int(r.randint(np_)), int(r.choice([0, 1, 2, 5, 10, 10, 10, 17]))))
    sg = [(5, 5, 5, 5, 0), (0, 0, 0, 0, 1), (w - 1, h - 1, w - 1, h - 1, 2), (-3, 4, -3, 4, 3), (w, h, w, h, 4)]   # zero length
    sg += [(2, 7, w - 3, 7, 0), (w - 3, 9, 2, 9, 1), (6, 1, 6, h - 2, 2), (8, h - 2, 8, 1, 3)]                     # horizontal, vertical
    d = min(w, h) - 4
    sg += [(1, 1, 1 + d, 1 + d, 4), (2 + d, 1 + d, 2, 1, 5), (1, 2 + d, 1 + d, 2, 6), (3 + d, 1, 3, 1 + d, 0)]     # exact diagonals
    sg += [(10, 0, 13, h - 1, 1), (17, h - 1, 12, 0, 2), (0, 10, w - 1, 14, 3), (w - 1, 20, 0, 13, 4)]             # steep / shallow
    sg += [(-20, -9, w + 15, h + 30, 5), (w + 40, -7, -33, h + 5, 6), (-15, h // 2, w + 15, h // 2 + 1, 0),        # outside to outside
           (w // 2, -30, w // 2 - 1, h + 30, 1), (w + 9, h + 9, -9, -9, 2)]
    sg += [(-8191, -8191, 8191, 8191, 3), (8191, -8191, -8191, 8191, 4), (-8191, h // 2, 8191, h // 2 + 3, 5), (w // 3, 8191, w // 3 + 2, -8191, 6),
           (-8192, -8192, 8191, 8191, 0), (8191, 8191, 8000, 8100, 1), (-8191, 3, -8000, 9, 2)]                   # coordinates at the limits
    for o in range(8):                                                                                             # every octant, both signs
        dx, dy = [(9, 4), (4, 9), (-4, 9), (-9, 4), (-9, -4), (-4, -9), (4, -9), (9, -4)][o]
        sg.append((w // 2, h // 2, w // 2 + dx, h // 2 + dy, o % np_))
    while len(sg) < 400:
        sg.append((int(r.randint(-10, w + 10)), int(r.randint(-10, h + 10)), int(r.randint(-10, w + 10)), int(r.randint(-10, h + 10)), int(r.randint(np_))))
    assert len(mk) == 200 and len(sg) == 400
    return sg, mk


@functools.lru_cache(maxsize=None)
def _case(w, h):
    """gray frame, primitives and the model's answers (forward and reversed lists, BGRA) for a size -- computed once, never modified"""
    g = noise_image(w, h, seed=w + h)
    sg, mk = _primitives(w, h)
    fwd = vm.render(g, sg, mk, PALETTE, 4)
    rev = vm.render(g, sg[::-1], mk[::-1], PALETTE, 4)
    for a in (g, fwd, rev):
        a.setflags(write=False)
    return g, sg, mk, fwd, rev


def _want(model4, channels):
    return model4 if channels == 4 else model4[:, :, :3]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("channels", [3, 4])
def test_render_equals_the_model(klt, hbm, w, h, channels):
    """Host destination at strides w*c, w*c + 5, w*c + 64 (padding untouched); HBM destination at base offsets 0..3; the reversed lists."""
    g, sg, mk, fwd, rev = _case(w, h)
    ctx = klt.KltContext(w, h, 50)
    im = ctx.image(g)
    for pad in (0, 5, 64):
        stride = w * channels + pad
        buf = np.full(h * stride + 8, POISON, np.uint8)
        out = im.render_view(sg, mk, PALETTE, channels, stride, out=buf)
        np.testing.assert_array_equal(out, _want(fwd, channels), err_msg="host, stride w*c + %d" % pad)
        assert (buf[:h * stride].reshape(h, stride)[:, w * channels:] == POISON).all() and (buf[h * stride:] == POISON).all(), \
            "bytes outside the rows were written"
    np.testing.assert_array_equal(im.render_view(sg[::-1], mk[::-1], PALETTE, channels), _want(rev, channels), err_msg="reversed lists")
    assert (fwd != rev).any()
    for off in (0, 1, 2, 3):
        for pad in (0, 5):
            stride = w * channels + pad
            nbytes = off + h * stride + 16
            dev = hbm.alloc(nbytes, POISON)
            im.render_view(sg, mk, PALETTE, channels, stride, out=dev + off, on_device=True)
            ctx.synchronize()
            got = hbm.read(dev, nbytes)
            body = np.lib.stride_tricks.as_strided(got[off:], shape=(h, w, channels), strides=(stride, channels, 1))
            np.testing.assert_array_equal(body, _want(fwd, channels), err_msg="HBM, base offset %d, stride w*c + %d" % (off, pad))
            mask = np.ones(nbytes, bool)
            for y in range(h):
                mask[off + y * stride: off + y * stride + w * channels] = False
            assert (got[mask] == POISON).all(), "bytes outside the rows were written (base offset %d)" % off
    # the empty lists: the canvas alone
    canvas = vm.render(g, channels=channels)
    np.testing.assert_array_equal(im.render_view(channels=channels), canvas)
    np.testing.assert_array_equal(im.render_view(sg[:0], mk[:3], PALETTE, channels), vm.render(g, [], mk[:3], PALETTE, channels))
    np.testing.assert_array_equal(im.render_view(sg[:9], mk[:0], PALETTE, channels), vm.render(g, sg[:9], [], PALETTE, channels))


def test_canvas_sources(klt):
    """The canvas is the plane preprocess() reads: after upload, upload_color, upload_distorted (== raw()), and CLAHE leaves it alone."""
    from oracle import undistort as ou
    w, h = 752, 480
    g = noise_image(w, h, seed=9)
    ctx = klt.KltContext(w, h, 50)
    im = ctx.image(g)
    mk = [(100, 100, 0, 10)]
    np.testing.assert_array_equal(im.render_view([], mk, PALETTE), vm.render(g, [], mk, PALETTE))
    px = cf.colorize(g, 3, pad=5)
    im.upload_color(px)
    np.testing.assert_array_equal(im.render_view([], mk, PALETTE, 4), vm.render(cf.gray_ref(px), [], mk, PALETTE, 4))
    ctx.set_undistort_map(ou.packed_map(w, h, (458.654, 457.296, 367.215, 248.375), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05), "radtan"))
    im.upload_distorted(g)
    raw = im.raw()
    assert (raw != g).mean() > 0.5
    np.testing.assert_array_equal(im.render_view([], mk, PALETTE), vm.render(raw, [], mk, PALETTE))
    im.preprocess()
    np.testing.assert_array_equal(im.render_view([], mk, PALETTE), vm.render(raw, [], mk, PALETTE), err_msg="after preprocess (CLAHE)")
    assert (im.level(0)[0] != raw).any()


def test_errors(klt):
    from xrslam_amd import _lib
    C = klt.C
    w, h = 96, 67
    ctx = klt.KltContext(w, h, 50)
    g = noise_image(w, h, seed=2)
    im = ctx.image(g)
    L = klt.L()
    out = np.zeros(h * w * 4, np.uint8)
    pal = np.array(PALETTE, np.uint8)
    seg = np.array([[1, 2, 30, 40, 1]], np.int32)
    mkr = np.array([[5, 6, 2 | (10 << 8)]], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def rc(img=im._h, segs=p(seg), ns=1, mks=p(mkr), nm=1, pl=p(pal), npal=len(PALETTE), o=p(out), stride=w * 3, ch=3):
        return L.xrhip_image_render_view(img, segs, ns, mks, nm, pl, npal, o, stride, ch, 0)

    assert rc() == 0
    for kw in (dict(img=None), dict(o=None), dict(segs=None), dict(mks=None), dict(pl=None)):
        assert rc(**kw) == _lib.XRHIP_EINVAL, kw
    for ch in (0, 1, 2, 5, -3):
        assert rc(ch=ch, stride=w * 8) == _lib.XRHIP_EINVAL
    assert rc(stride=w * 3 - 1) == _lib.XRHIP_EINVAL
    assert rc(stride=w * 4 - 1, ch=4) == _lib.XRHIP_EINVAL
    assert b"stride" in _lib.lib().xrhip_last_error()
    assert rc(npal=1) == _lib.XRHIP_EINVAL                      # the segment's palette index 1 >= n_palette
    assert rc(npal=2) == _lib.XRHIP_EINVAL                      # the marker's 2
    assert b"palette" in _lib.lib().xrhip_last_error()
    assert rc(npal=3) == 0
    assert rc(npal=257) == _lib.XRHIP_EINVAL
    for col in range(4):
        for v in (8192, -8193, 100000, -2 ** 31):
            bad = seg.copy()
            bad[0, col] = v
            assert rc(segs=p(bad)) == _lib.XRHIP_EINVAL, (col, v)
    for col in range(2):
        for v in (8192, -8193):
            bad = mkr.copy()
            bad[0, col] = v
            assert rc(mks=p(bad)) == _lib.XRHIP_EINVAL, (col, v)
    assert b"coordinate" in _lib.lib().xrhip_last_error()
    lim = np.array([[-8192, 8191, 8191, -8192, 0]], np.int32)
    assert rc(segs=p(lim)) == 0
    # the renderer still answers, and answers right, after the refusals
    np.testing.assert_array_equal(im.render_view([(1, 2, 30, 40, 1)], [(5, 6, 2, 10)], PALETTE),
                                  vm.render(g, [(1, 2, 30, 40, 1)], [(5, 6, 2, 10)], PALETTE))
    im.release_image_buffer()
    assert rc() == _lib.XRHIP_ESTATE
    fresh = ctx.image()
    assert rc(img=fresh._h) == _lib.XRHIP_ESTATE                # never uploaded
    im.upload(g)
    assert rc() == 0


def test_a_render_does_not_disturb_the_tracker(klt):
    """preprocess / detect / track on a context that rendered first give the answers of a context that never rendered."""
    from tests.util import warp_affine
    w, h = 352, 353
    a = noise_image(w, h, seed=21)
    b = warp_affine(a, np.eye(2), np.array([1.25, -0.75]))
    res = []
    for render in (True, False):
        ctx = klt.KltContext(w, h, 100)
        A, B = ctx.image(a), ctx.image(b)
        if render:
            sg, mk = _primitives(w, h)
            A.render_view(sg, mk, PALETTE)
        A.preprocess()
        B.preprocess()
        if render:
            B.render_view([], [(10, 10, 0, 10)], PALETTE, 4)
        kp = A.detect_keypoints(np.zeros((0, 2)), 100, 20.0)
        nx, st = A.track_keypoints(B, kp, None)
        res.append((A.level(0)[0], A.level(3)[1], kp, nx, st))
        ctx.synchronize()
    for x, y in zip(*res):
        np.testing.assert_array_equal(x, y)
    assert len(res[0][2]) > 20 and res[0][4].sum() > 10
