"""GPU parity of the Lucas-Kanade PARAMETERS (xrhip_klt_set_lk_params): window, pyramid depth, iteration cap, epsilon.  The kernels
with runtime parameters (klt_kernels.hip.h: k_scharr_level, k_lk_track_g, k_lk_plain_g) against the CPU oracle at the same values, bit
for bit: every pyramid level with its 21-pixel border and its derivatives, plain LK positions and status with the template / iteration
counts, and xrhip_image_track against tests/lk_params_model.py (orc_track_keypoints with the parameters as arguments;
tests/test_lk_params_model.py pins it).  At the reference's values with the development switch on they must also equal the
specialised kernels.

Every figure asserted on the ORACLE's side only keeps a comparison from passing empty; the device result is always compared with
assert_array_equal."""
import ctypes as C

import numpy as np
import pytest

from tests import lk_params_model as lm
from tests.util import constant_image, noise_image, shifted

pytestmark = pytest.mark.gpu

SEED = 21
NONE = np.zeros((0, 2))
# (tag, frame size, (win, max_level, max_count, epsilon), development switch, frame shift)
POINTS = [
    ("reference_forced", (416, 352), (21, 3, 30, 0.01), True, (3, -2)),
    ("win21_level4", (401, 347), (21, 4, 30, 0.01), False, (3, -2)),          # top level 26 x 22
    ("win9_level5", (416, 352), (9, 5, 30, 0.01), False, (3, -2)),            # top level 13 x 11
    ("win5_level0", (416, 352), (5, 0, 30, 0.01), False, (3, -2)),
    ("win15_level2_cap5", (401, 347), (15, 2, 5, 0.3), False, (3, -2)),       # iteration-cap exits dominate
    ("win11_cap100_eps0", (416, 352), (11, 3, 100, 0.0), False, (3, -2)),
    ("win7_level1_64x64", (64, 64), (7, 1, 30, 0.01), False, (1.5, 0.5)),
]
IDS = [p[0] for p in POINTS]


@pytest.fixture(scope="module")
def klt():
    from xrslam_amd import klt
    return klt


_frames = {}


def _frame(w, h):
    if (w, h) not in _frames:
        g = noise_image(w, h, seed=SEED)
        g.setflags(write=False)
        _frames[w, h] = g
    return _frames[w, h]


class Case:
    """One parameter point: a context with the parameters set, a frame and its shifted copy preprocessed on the device and by the
    oracle (once per module)."""

    def __init__(self, klt, point):
        self.tag, (self.w, self.h), self.params, self.forced, self.shift = point
        self.ctx = klt.KltContext(self.w, self.h, 150)
        self.ctx.set_lk_params(*self.params)
        self.ctx.force_general_lk(self.forced)
        self.ctx.set_profiling(True)
        self.g = _frame(self.w, self.h)
        self.g2 = shifted(self.g, *self.shift)
        self.HA, self.HB = self.ctx.image(self.g), self.ctx.image(self.g2)
        self.HA.preprocess()
        self.HB.preprocess()
        self.OA, self.OB = lm.oracle_image(self.g, self.params[1]), lm.oracle_image(self.g2, self.params[1])

    def lk_kw(self):
        win, max_level, max_count, eps = self.params
        return dict(win=win, max_level=max_level, max_count=max_count, eps=eps)


_cases = {}


@pytest.fixture(scope="module")
def case(klt):
    def get(point):
        if point[0] not in _cases:
            _cases[point[0]] = Case(klt, point)
        return _cases[point[0]]

    yield get
    _cases.clear()


def _assert_lk(c, pts, guess, tag):
    """Plain LK, positions and status; the device's template / iteration counters against OrcLkStats."""
    nx_o, st_o, stats = c.OA.lk(c.OB, pts, guess, **c.lk_kw())
    c.ctx.stats(reset=True)
    nx_h, st_h = c.HA.lk(c.HB, pts, guess)
    s = c.ctx.stats()
    np.testing.assert_array_equal(st_h, st_o, err_msg=tag + " status")
    np.testing.assert_array_equal(nx_h, nx_o, err_msg=tag + " positions")
    assert (s.lk_templates, s.lk_iterations) == (stats.templates, stats.iters), tag
    return nx_o, st_o, stats


def _assert_track(c, pts, guess, tag, H=None):
    HA, HB = H or (c.HA, c.HB)
    nx_o, st_o = lm.track_keypoints(c.OA, c.OB, pts, guess, *c.params)
    c.ctx.stats(reset=True)
    nx_h, st_h = HA.track_keypoints(HB, pts, guess)
    np.testing.assert_array_equal(st_h, st_o, err_msg=tag + " status")
    np.testing.assert_array_equal(nx_h, nx_o, err_msg=tag + " positions")
    assert c.ctx.stats().lk_points == len(pts)
    return nx_o, st_o


@pytest.mark.parametrize("point", POINTS, ids=IDS)
def test_pyramid_levels(case, point):
    """Levels 0 .. max_level of both frames: image, derivatives, and the plane with its 21-pixel reflect-101 border (several
    reflections per border pixel on the 13 x 11 and 26 x 22 top levels); a level past max_level does not exist."""
    from xrslam_amd._lib import XRHIP_EINVAL, XrhipError
    c = case(point)
    assert c.ctx.get_lk_params() == c.params
    for H, O in ((c.HA, c.OA), (c.HB, c.OB)):
        for l in range(c.params[1] + 1):
            hi, hd = H.level(l)
            oi, od = O.level(l)
            op, _ = O.level(l, padded=True)
            assert hi.shape == oi.shape, (c.tag, l)
            np.testing.assert_array_equal(hi, oi, err_msg="%s level %d image" % (c.tag, l))
            np.testing.assert_array_equal(hd, od, err_msg="%s level %d derivatives" % (c.tag, l))
            np.testing.assert_array_equal(H.level_padded(l), op, err_msg="%s level %d padded plane" % (c.tag, l))
    with pytest.raises(XrhipError) as e:
        c.HA.level(c.params[1] + 1)
    assert e.value.code == XRHIP_EINVAL


def test_deeper_pyramid_extends_the_default_one(klt, case):
    """The first four levels at max_level 5 are the default (fused, specialised) pyramid's."""
    c = case(POINTS[2])
    ctx = klt.KltContext(c.w, c.h, 150)
    D = ctx.image(c.g)
    D.preprocess()
    for l in range(4):
        np.testing.assert_array_equal(c.HA.level_padded(l), D.level_padded(l))
        np.testing.assert_array_equal(c.HA.level(l)[1], D.level(l)[1])


@pytest.mark.parametrize("point", POINTS, ids=IDS)
def test_plain_lk(case, point):
    """Points anywhere in and up to 24 pixels round the frame (templates within `win` of each border, outside it, and past the -win
    bound), guesses a few pixels off; guesses far outside the image; and guesses 6 - 9 pixels (times 2^max_level: the same at the
    top level) off the true position along +-x and +-y on a grid whose x covers every residue mod 4 -- the search tile reaches 5
    pixels round the level's starting position, so the iterations start beyond it in each direction and read global memory."""
    c = case(point)
    w, h, (sx, sy) = c.w, c.h, c.shift
    rng = np.random.RandomState(w * 1000 + h + c.params[0])
    pts = (rng.rand(200, 2) * [w + 48, h + 40] - [24, 20]).astype(np.float32)
    guess = (pts + [sx, sy] + rng.uniform(-3, 3, pts.shape)).astype(np.float32)
    _, st, stats = _assert_lk(c, pts, guess, c.tag + " scattered")
    assert 0 < st.sum() < len(st) and stats.iters > 0
    far = guess.copy()
    far[0::4] = [-100.0, -100.0]
    far[1::4] = [w + 200.0, 50.0]
    far[2::4, 1] = h + 150.0
    _, st, _ = _assert_lk(c, pts, far, c.tag + " guesses outside the image")
    assert 0 < st.sum() < len(st)
    n = 16 if w > 64 else 4
    ii, jj = np.meshgrid(np.arange(n), np.arange(n))
    step = (((w - 80) // n) | 1, (h - 80) // n) if w > 64 else (5, 5)      # (an odd step in x: every residue mod 4)
    grid = np.stack([40 + step[0] * ii.ravel(), 40 + step[1] * jj.ravel()], axis=1).astype(np.float32)
    if w == 64:
        grid = grid - 16
    assert sorted(set(grid[:, 0].astype(int) % 4)) == [0, 1, 2, 3]
    true = grid + np.array([sx, sy], np.float32)
    ok = 0
    for scale in sorted({1, 1 << c.params[1]}):
        for d in (6, 9):
            for axis in (0, 1):
                for sign in (1, -1):
                    off = np.zeros(2, np.float32)
                    off[axis] = sign * d * scale
                    _, st, _ = _assert_lk(c, grid, true + off, "%s guess %+d along %s" % (c.tag, sign * d * scale, "xy"[axis]))
                    ok += int(st.sum())
    assert ok > 0


@pytest.mark.parametrize("point", POINTS, ids=IDS)
def test_track(case, point):
    """xrhip_image_track against the model: 1, 160 and 161 points (either side of the specialised path's inline limit), with and
    without a guess; corners first, then points anywhere in the frame (the 20-pixel border gate, failed round trips)."""
    c = case(point)
    w, h = c.w, c.h
    kp = c.OA.detect_keypoints(NONE, 150, 20.0)
    rng = np.random.RandomState(6)
    pts = np.concatenate([kp, rng.rand(161, 2) * [w - 1, h - 1]], axis=0)[:161]
    if w == 64:
        pts = rng.rand(161, 2) * [w - 1, h - 1]
    guesses = pts + np.array(c.shift, np.float64) + rng.uniform(-1, 1, pts.shape)
    res = {}
    for n in (1, 160, 161):
        for has in (0, 1):
            res[n, has] = _assert_track(c, pts[:n], guesses[:n] if has else None, "%s n = %d guess %d" % (c.tag, n, has))
    assert 0 < res[161, 1][1].sum() < 161
    if c.forced:   # the reference's values on the general path: also what orc_track_keypoints and the specialised kernels give
        D = type(c.ctx)(w, h, 150)
        DA, DB = D.image(c.g), D.image(c.g2)
        DA.preprocess()
        DB.preprocess()
        for has in (0, 1):
            g = guesses if has else None
            nx_o, st_o = c.OA.track_keypoints(c.OB, pts, g)
            nx_d, st_d = DA.track_keypoints(DB, pts, g)
            for nx, st in ((nx_o, st_o), (nx_d, st_d)):
                np.testing.assert_array_equal(st, res[161, has][1])
                np.testing.assert_array_equal(nx, res[161, has][0])
        lp = pts.astype(np.float32)
        nx_g, st_g = c.HA.lk(c.HB, lp, guesses.astype(np.float32))
        nx_d, st_d = DA.lk(DB, lp, guesses.astype(np.float32))
        np.testing.assert_array_equal(st_g, st_d)
        np.testing.assert_array_equal(nx_g, nx_d)


@pytest.mark.parametrize("point", [POINTS[2], POINTS[4]], ids=[IDS[2], IDS[4]])
def test_constant_frame_fails_every_point_at_the_eigenvalue_gate(case, point):
    c = case(point)
    flat = constant_image(c.w, c.h, 110)
    FA, FB = c.ctx.image(flat), c.ctx.image(flat)
    FA.preprocess()
    FB.preprocess()
    OA, OB = lm.oracle_image(flat, c.params[1]), lm.oracle_image(flat, c.params[1])
    rng = np.random.RandomState(9)
    pts = (rng.rand(100, 2) * [c.w - 60, c.h - 60] + 30).astype(np.float32)
    nx_o, st_o, stats = OA.lk(OB, pts, pts + 1, **c.lk_kw())
    assert not st_o.any() and stats.iters == 0 and stats.templates == 100 * (c.params[1] + 1)
    c.ctx.stats(reset=True)
    nx_h, st_h = FA.lk(FB, pts, pts + 1)
    s = c.ctx.stats()
    np.testing.assert_array_equal(st_h, st_o)
    np.testing.assert_array_equal(nx_h, nx_o)
    assert (s.lk_templates, s.lk_iterations) == (stats.templates, 0)
    nx_t, st_t = FA.track_keypoints(FB, pts.astype(np.float64))
    nx_m, st_m = lm.track_keypoints(OA, OB, pts.astype(np.float64), None, *c.params)
    np.testing.assert_array_equal(st_t, st_m)
    np.testing.assert_array_equal(nx_t, nx_m)
    FA.close()
    FB.close()


def test_large_motion_needs_the_deeper_pyramid(klt):
    """A frame moved by 56 pixels, 9-pixel window, no guess: with max_level 5 the oracle keeps 91 of its 111 corners, with 3 it keeps
    32 (chosen with the oracle alone).  The device equals the model at both depths."""
    w, h = 416, 352
    g = _frame(w, h)
    g2 = shifted(g, 56, 0)
    kept = {}
    for max_level in (3, 5):
        params = (9, max_level, 30, 0.01)
        OA, OB = lm.oracle_image(g, max_level), lm.oracle_image(g2, max_level)
        kp = OA.detect_keypoints(NONE, 150, 20.0)
        nx_o, st_o = lm.track_keypoints(OA, OB, kp, None, *params)
        ctx = klt.KltContext(w, h, 150)
        ctx.set_lk_params(*params)
        HA, HB = ctx.image(g), ctx.image(g2)
        HA.preprocess()
        HB.preprocess()
        nx_h, st_h = HA.track_keypoints(HB, kp)
        np.testing.assert_array_equal(st_h, st_o)
        np.testing.assert_array_equal(nx_h, nx_o)
        kept[max_level] = int(st_o.sum())
        n = len(kp)
    assert kept[5] != kept[3] and kept[5] >= n // 2, (kept, n)      # a guard against an empty comparison, not a tolerance


BAD = [
    ("even win", dict(win=20)),
    ("win 23", dict(win=23)),
    ("win 3", dict(win=3)),
    ("max_level 6", dict(max_level=6)),
    ("max_level -1", dict(max_level=-1)),
    ("top level not larger than the window", dict(win=21, max_level=5)),      # 752 x 480: level 5 is 24 x 15
    ("max_count 0", dict(max_count=0)),
    ("max_count 101", dict(max_count=101)),
    ("negative epsilon", dict(epsilon=-0.5)),
    ("epsilon 11", dict(epsilon=11.0)),
    ("epsilon nan", dict(epsilon=float("nan"))),
]


def test_argument_errors_leave_the_context_as_it_was(klt):
    """Each bad value: XRHIP_EINVAL with the field's name in the message, get_lk_params unchanged.  Parameters after an image
    exists, parameters on a member of a group, a non-default context joining a group: XRHIP_ESTATE.  After all of them a default
    track on the same context still equals the oracle."""
    from oracle import klt_oracle as ko
    from xrslam_amd import _lib
    from xrslam_amd._lib import XRHIP_EINVAL, XRHIP_ESTATE, XrhipError
    w, h = 752, 480
    ctx = klt.KltContext(w, h, 150)
    assert ctx.get_lk_params() == klt.LK_DEFAULTS
    ctx.set_lk_params(15, 2, 10, 0.05)
    assert ctx.get_lk_params() == (15, 2, 10, 0.05)
    ctx.set_lk_params()
    assert ctx.get_lk_params() == klt.LK_DEFAULTS
    field = {"win": "win", "max_level": "max_level", "max_count": "max_count", "epsilon": "epsilon"}
    for tag, kw in BAD:
        with pytest.raises(XrhipError) as e:
            ctx.set_lk_params(**kw)
        assert e.value.code == XRHIP_EINVAL, tag
        assert field[list(kw)[-1]] in str(e.value), (tag, str(e.value))
        assert ctx.get_lk_params() == klt.LK_DEFAULTS, tag
    lib = _lib.lib()
    lib.xrhip_group_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.xrhip_group_destroy.argtypes = [C.c_void_p]
    lib.xrhip_klt_join_group.argtypes = [C.c_void_p, C.c_void_p]
    group = C.c_void_p()
    assert lib.xrhip_group_create(C.byref(group)) == 0
    try:
        other = klt.KltContext(w, h, 150)
        other.set_lk_params(15, 2)
        assert lib.xrhip_klt_join_group(other._h, group) == XRHIP_ESTATE
        assert b"LK parameters" in lib.xrhip_last_error()
        other.close()
        assert lib.xrhip_klt_join_group(ctx._h, group) == 0, lib.xrhip_last_error()
        with pytest.raises(XrhipError) as e:
            ctx.set_lk_params(15, 2)
        assert e.value.code == XRHIP_ESTATE
        with pytest.raises(XrhipError) as e:
            ctx.force_general_lk(True)
        assert e.value.code == XRHIP_ESTATE
        assert lib.xrhip_klt_join_group(ctx._h, None) == 0
    finally:
        lib.xrhip_group_destroy(group)
    g = noise_image(w, h, seed=SEED)
    g2 = shifted(g, 3, -2)
    HA, HB = ctx.image(g), ctx.image(g2)
    with pytest.raises(XrhipError) as e:
        ctx.set_lk_params(15, 2)
    assert e.value.code == XRHIP_ESTATE and "images" in str(e.value)
    assert ctx.get_lk_params() == klt.LK_DEFAULTS
    HA.preprocess()
    HB.preprocess()
    OA, OB = ko.OracleImage(g), ko.OracleImage(g2)
    OA.preprocess()
    OB.preprocess()
    kp = OA.detect_keypoints(NONE, 150, 20.0)
    nx_o, st_o = OA.track_keypoints(OB, kp)
    nx_h, st_h = HA.track_keypoints(HB, kp)
    assert st_o.sum() >= 80
    np.testing.assert_array_equal(st_h, st_o)
    np.testing.assert_array_equal(nx_h, nx_o)
    HA.close()
    HB.close()
    ctx.set_lk_params(15, 2)                     # no images left: accepted again
    assert ctx.get_lk_params() == (15, 2, 30, 0.01)
