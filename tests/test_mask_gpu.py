"""Masks on the device (include/xrslam_hip.h, "Masks"): the effective plane k_mask_ingest writes, detection under a mask against
tests/mask_model.py (which tests/test_mask_model.py pins to the CPU oracle), the track gate against the oracle's tracks followed by the
model's gate, the all-ones identity and the group rules.

Two contexts: 320 x 240, and 202 x 137 -- no multiple of the 64 x 16 Harris tile (tile edges and the clamped ring are live), a width
that is no multiple of 4 (k_mask_ingest's row-straddling dwords) and a pixel count that is none either (its tail).

Figures asserted on the model's / oracle's side only keep a comparison from passing empty; device results are compared with
assert_array_equal."""
import ctypes as C

import numpy as np
import pytest

from oracle import klt_oracle as ko
from tests import lk_params_model as lm
from tests import mask_model as mm
from tests.color_frames import Hbm
from tests.util import noise_image, shifted

pytestmark = pytest.mark.gpu

SIZES = [(320, 240), (202, 137)]
SIZE_IDS = ["320x240", "202x137"]
NONE = np.zeros((0, 2))


@pytest.fixture(scope="module")
def klt():
    from xrslam_amd import klt
    return klt


@pytest.fixture(scope="module")
def hbm():
    m = Hbm()
    yield m
    m.close()


class Scene:
    """A context, a frame and its shifted copy on the device and in the oracle, the frame's Harris plane (once per module)."""

    def __init__(self, klt, w, h, lk=None):
        self.w, self.h = w, h
        self.ctx = klt.KltContext(w, h, 150)
        if lk:
            self.ctx.set_lk_params(*lk)
        self.g = noise_image(w, h, seed=31 + w)
        self.g2 = shifted(self.g, 3, -2)
        self.A, self.B = self.ctx.image(self.g), self.ctx.image(self.g2)
        self.A.preprocess()
        self.B.preprocess()
        self.resp = self.A.harris()
        self.resp_b = self.B.harris()
        level = lk[1] if lk else 3
        self.OA, self.OB = lm.oracle_image(self.g, level), lm.oracle_image(self.g2, level)
        self.lk = lk or (21, 3, 30, 0.01)
        rs = np.random.RandomState(w)
        self.exist = np.stack([rs.uniform(15, w - 15, 30), rs.uniform(15, h - 15, 30)], axis=1)

    def load(self, im, g, mask, **how):
        """The frame `g` with the per-frame mask `mask` (None: none), preprocessed"""
        im.upload(g)
        if mask is not None:
            im.set_mask(mask, **how)
        im.preprocess()
        return im


_scenes = {}


@pytest.fixture(scope="module")
def scene(klt):
    def get(size, lk=None):
        if (size, lk) not in _scenes:
            _scenes[size, lk] = Scene(klt, size[0], size[1], lk)
        return _scenes[size, lk]

    yield get
    _scenes.clear()


def random_mask(w, h, seed, values=(0, 1, 128, 255)):
    return np.random.RandomState(seed).choice(np.array(values, np.uint8), size=(h, w))


def padded(mask, pad, offset):
    """The same mask as a view with rows `pad` bytes longer, starting `offset` bytes into its buffer (other bytes: 0 / 255 noise)"""
    h, w = mask.shape
    buf = np.random.RandomState(7).choice(np.array([0, 255], np.uint8), size=offset + h * (w + pad))
    view = buf[offset:].reshape(h, w + pad)[:, :w]
    view[:] = mask
    return view


def give(hbm, mask, where, pad, offset):
    """-> keyword arguments of set_mask for `mask` on the host or in HBM, dense or padded at an odd base offset"""
    view = padded(mask, pad, offset) if pad or offset else np.ascontiguousarray(mask)
    if where == "host":
        return dict(mask=view)
    return dict(mask=hbm.put(view, offset=offset), on_device=True, stride=view.strides[0])


LAYOUTS = [("host", 0, 0), ("host", 5, 1), ("hbm", 0, 0), ("hbm", 7, 3), ("hbm", 0, 1)]


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=["%s_pad%d_off%d" % l for l in LAYOUTS])
def test_effective_plane(klt, scene, hbm, size, layout):
    """xrhip_debug_get_mask == (static != 0) & (per_frame != 0) for static only, per-frame only and both; 1, 128 and 255 are one value."""
    s = scene(size)
    where, pad, offset = layout
    ms, mp = random_mask(s.w, s.h, 1), random_mask(s.w, s.h, 2)
    im = s.ctx.image()
    try:
        im.upload(s.g)
        im.set_mask(**give(hbm, mp, where, pad, offset))
        np.testing.assert_array_equal(im.mask(), (mp != 0).astype(np.uint8), err_msg="per-frame only")
        s.ctx.set_mask(**give(hbm, ms, where, pad, offset))
        im.upload(s.g)
        np.testing.assert_array_equal(im.mask(), (ms != 0).astype(np.uint8), err_msg="static only")
        im.upload(s.g)
        im.set_mask(**give(hbm, mp, where, pad, offset))
        np.testing.assert_array_equal(im.mask(), ((ms != 0) & (mp != 0)).astype(np.uint8), err_msg="both")
        im.set_mask(None)
        np.testing.assert_array_equal(im.mask(), (ms != 0).astype(np.uint8), err_msg="per-frame cleared")
    finally:
        s.ctx.set_mask(None)
        im.close()
    assert 0 < int((ms != 0).sum()) < ms.size


def test_per_frame_mask_is_gone_after_the_next_upload(klt, scene):
    from xrslam_amd._lib import XRHIP_ESTATE, XrhipError
    s = scene(SIZES[0])
    im = s.ctx.image(s.g)
    with pytest.raises(XrhipError) as e:
        im.mask()
    assert e.value.code == XRHIP_ESTATE
    im.set_mask(random_mask(s.w, s.h, 3))
    assert im.mask().shape == (s.h, s.w)
    im.upload(s.g)
    with pytest.raises(XrhipError) as e:
        im.mask()
    assert e.value.code == XRHIP_ESTATE and "no mask" in str(e.value)
    im.close()


def masks_of(s):
    """name -> mask of the scene's size"""
    w, h = s.w, s.h
    ones = np.ones((h, w), np.uint8)
    out = {"ones": ones, "zero": np.zeros((h, w), np.uint8)}
    m = ones.copy()
    m[:, :w // 2] = 0
    out["left_half"] = m
    my, mx = np.unravel_index(np.argmax(s.resp), s.resp.shape)
    m = ones.copy()
    m[max(my - 25, 0):my + 26, max(mx - 25, 0):mx + 26] = 0
    out["hide_max"] = m
    out["checker"] = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255).astype(np.uint8)
    m = ones.copy()
    m[:, 63:65] = 0
    m[:, 127:129] = 0
    m[15:17, :] = 0
    m[127:129, :] = 0
    out["seams"] = m
    m = ones.copy()
    m[20:h - 20, 20:w - 20] = 0
    out["border_only"] = m
    return out


KINDS = ["ones", "zero", "left_half", "hide_max", "checker", "seams", "border_only"]


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_detection_equals_the_model(klt, scene, size, kind):
    s = scene(size)
    mask = masks_of(s)[kind]
    s.load(s.A, s.g, mask)
    n_model = 0
    for ex in (NONE, s.exist):
        for max_points in (150, 20):
            want = mm.detect(s.resp, mask, ex, max_points, 20.0)
            got = s.A.detect_keypoints(ex, max_points, 20.0)
            np.testing.assert_array_equal(got[:len(ex)], ex)
            np.testing.assert_array_equal(got[len(ex):], want, err_msg="%s, %d existing, max %d" % (kind, len(ex), max_points))
            n_model += len(want)
    assert (n_model == 0) == (kind in ("zero", "border_only")), n_model
    if kind == "hide_max":
        assert mm.threshold(s.resp, mask) < mm.threshold(s.resp, np.ones_like(mask))
    # the pass leaves the context's running maximum and counters reset: an unmasked detection behind it is the oracle's
    s.load(s.A, s.g, None)
    np.testing.assert_array_equal(s.A.detect_keypoints(NONE, 150, 20.0), s.OA.detect_keypoints(NONE, 150, 20.0))


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_static_mask_detection_equals_the_model(klt, scene, size):
    s = scene(size)
    mask = masks_of(s)["left_half"]
    s.ctx.set_mask(mask)
    try:
        s.load(s.A, s.g, None)
        want = mm.detect(s.resp, mask, s.exist, 150, 20.0)
        np.testing.assert_array_equal(s.A.detect_keypoints(s.exist, 150, 20.0)[len(s.exist):], want)
        assert len(want) > 0
    finally:
        s.ctx.set_mask(None)
    s.load(s.A, s.g, None)


def track_points(s, n_more):
    """Corners of A plus n_more positions off the pixel grid (any position can be tracked on the noise frame)"""
    s.load(s.A, s.g, None)
    pts = s.A.detect_keypoints(NONE, 150, 20.0)
    rs = np.random.RandomState(11)
    more = np.stack([rs.uniform(30, s.w - 30, n_more), rs.uniform(30, s.h - 30, n_more)], axis=1)
    return np.concatenate([pts, more], axis=0)


def boundary_mask(s, nx, st):
    """A vertical mask boundary through the middle of the tracked points: the left side is excluded"""
    m = np.ones((s.h, s.w), np.uint8)
    m[:, :int(np.median(nx[st != 0, 0]))] = 0
    return m


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("kind", ["ones", "left_half", "seams"])
def test_prefetched_detection_equals_the_model(klt, scene, size, kind):
    """The Harris pass of `next` riding behind the tracking launch uses next's mask"""
    s = scene(size)
    mask = masks_of(s)[kind]
    pts = track_points(s, 0)
    s.load(s.B, s.g2, mask)
    s.B.prefetch_detect()
    nx, st = s.A.track_keypoints(s.B, pts)
    got = s.B.detect_keypoints(s.exist, 150, 20.0)[len(s.exist):]
    want = mm.detect(s.resp_b, mask, s.exist, 150, 20.0)
    np.testing.assert_array_equal(got, want)
    assert len(want) > 0
    s.load(s.B, s.g2, None)


def assert_gated_track(s, n_more, tag):
    pts = track_points(s, n_more)
    if s.lk == (21, 3, 30, 0.01):
        nx_o, st_o = s.OA.track_keypoints(s.OB, pts)   # orc_track_keypoints
    else:
        nx_o, st_o = lm.track_keypoints(s.OA, s.OB, pts, None, *s.lk)
    mask = boundary_mask(s, nx_o, st_o)
    st_want = mm.track_gate(nx_o, st_o, mask)
    nx_want = nx_o.copy()
    nx_want[st_want == 0] = 0   # (a dropped point's position is not written)
    s.load(s.B, s.g2, mask)
    nx, st = s.A.track_keypoints(s.B, pts)
    np.testing.assert_array_equal(st, st_want, err_msg=tag + " status")
    np.testing.assert_array_equal(nx, nx_want, err_msg=tag + " positions")
    dropped = int(st_o.sum()) - int(st_want.sum())
    assert dropped > 5 and int(st_want.sum()) > 5, (tag, dropped, int(st_want.sum()))
    # cur's mask plays no part: all of A excluded changes nothing
    s.load(s.A, s.g, np.zeros((s.h, s.w), np.uint8))
    nx2, st2 = s.A.track_keypoints(s.B, pts)
    np.testing.assert_array_equal(st2, st_want, err_msg=tag + " status with cur masked")
    np.testing.assert_array_equal(nx2, nx_want, err_msg=tag + " positions with cur masked")
    # plain LK ignores masks
    p32 = pts.astype(np.float32)
    a, b = s.A.lk(s.B, p32, p32)
    s.load(s.A, s.g, None)
    s.load(s.B, s.g2, None)
    a0, b0 = s.A.lk(s.B, p32, p32)
    np.testing.assert_array_equal(a, a0)
    np.testing.assert_array_equal(b, b0)
    return len(pts)


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_track_gate_inline_points(klt, scene, size):
    assert assert_gated_track(scene(size), 0, "inline") <= 160


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_track_gate_pinned_points(klt, scene, size):
    assert assert_gated_track(scene(size), 170, "pinned") > 160


def test_track_gate_at_other_lk_parameters(klt, scene):
    assert_gated_track(scene(SIZES[0], (15, 2, 30, 0.01)), 40, "win15_level2")


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_an_all_ones_mask_changes_nothing(klt, scene, size):
    s = scene(size)
    pts = track_points(s, 60)
    s.load(s.A, s.g, None)
    s.load(s.B, s.g2, None)
    det0 = [s.A.detect_keypoints(ex, mp, 20.0) for ex in (NONE, s.exist) for mp in (150, 20)]
    nx0, st0 = s.A.track_keypoints(s.B, pts)
    ones = np.full((s.h, s.w), 255, np.uint8)
    for static in (False, True):
        if static:
            s.ctx.set_mask(ones)
        try:
            s.load(s.A, s.g, None if static else ones)
            s.load(s.B, s.g2, None if static else ones)
            assert s.B.mask().all()
            det1 = [s.A.detect_keypoints(ex, mp, 20.0) for ex in (NONE, s.exist) for mp in (150, 20)]
            nx1, st1 = s.A.track_keypoints(s.B, pts)
        finally:
            s.ctx.set_mask(None)
        for a, b in zip(det0, det1):
            assert a.tobytes() == b.tobytes()
        assert nx0.tobytes() == nx1.tobytes() and st0.tobytes() == st1.tobytes()
    assert int(st0.sum()) > 20 and len(det0[0]) > 20
    s.load(s.A, s.g, None)
    s.load(s.B, s.g2, None)


def test_bad_arguments_leave_the_mask_as_it_was(klt, scene):
    from xrslam_amd._lib import XRHIP_EINVAL, XrhipError
    s = scene(SIZES[0])
    m = masks_of(s)["left_half"]
    s.ctx.set_mask(m)
    try:
        with pytest.raises(XrhipError) as e:
            s.ctx.set_mask(np.ones((s.h, s.w), np.uint8), stride=s.w - 1)
        assert e.value.code == XRHIP_EINVAL and "stride" in str(e.value)
        im = s.ctx.image(s.g)
        np.testing.assert_array_equal(im.mask(), m)
        with pytest.raises(XrhipError) as e:
            im.set_mask(np.ones((s.h, s.w), np.uint8), stride=3)
        assert e.value.code == XRHIP_EINVAL and "stride" in str(e.value)
        np.testing.assert_array_equal(im.mask(), m)
        im.close()
    finally:
        s.ctx.set_mask(None)


def test_masks_and_groups_exclude_each_other(klt, scene):
    from xrslam_amd import _lib
    from xrslam_amd._lib import XRHIP_ESTATE, XrhipError
    w, h = SIZES[0]
    lib = _lib.lib()
    lib.xrhip_group_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.xrhip_group_destroy.argtypes = [C.c_void_p]
    lib.xrhip_klt_join_group.argtypes = [C.c_void_p, C.c_void_p]
    group = C.c_void_p()
    assert lib.xrhip_group_create(C.byref(group)) == 0
    ones = np.ones((h, w), np.uint8)
    g = noise_image(w, h, seed=31 + w)
    member = klt.KltContext(w, h, 150)
    try:
        masked = klt.KltContext(w, h, 150)
        masked.set_mask(ones)
        assert lib.xrhip_klt_join_group(masked._h, group) == XRHIP_ESTATE
        assert b"mask" in lib.xrhip_last_error()
        masked.set_mask(None)
        im = masked.image(g)
        im.set_mask(ones)
        assert lib.xrhip_klt_join_group(masked._h, group) == XRHIP_ESTATE   # handed a per-frame mask once
        im.close()
        masked.close()
        assert lib.xrhip_klt_join_group(member._h, group) == 0, lib.xrhip_last_error()
        with pytest.raises(XrhipError) as e:
            member.set_mask(ones)
        assert e.value.code == XRHIP_ESTATE and "group" in str(e.value)
        A = member.image(g)
        with pytest.raises(XrhipError) as e:
            A.set_mask(ones)
        assert e.value.code == XRHIP_ESTATE and "group" in str(e.value)
        # the member keeps working
        A.preprocess()
        O = ko.OracleImage(g)
        O.preprocess()
        np.testing.assert_array_equal(A.detect_keypoints(NONE, 150, 20.0), O.detect_keypoints(NONE, 150, 20.0))
        A.close()
        assert lib.xrhip_klt_join_group(member._h, None) == 0
    finally:
        member.close()
        lib.xrhip_group_destroy(group)
