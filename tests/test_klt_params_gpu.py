"""GPU parity of the KLT front end over its PARAMETERS and input ranges: the HIP path (through the C ABI) against the CPU oracle,
bit for bit -- planes with their 21-pixel borders, derivative planes, Harris response, corner lists, LK positions and status bytes.
tests/test_klt_gpu.py runs one point of this space (clip 6.0, square 8 x 8 / 4 x 4 grids, min_distance 20, mid-contrast frames);
this file runs the rest: the CLAHE clip / grid space (tests/test_oracle_klt.py pins the oracle's CLAHE on the same grid against an
independent model), the frame sizes round the fused-pyramid switch and down to the 64 x 64 minimum, full-range derivatives, LK
iterations that leave the staged search tile in every direction and at every alignment, the point counts round the inline limit of
xrhip_image_track, and the detection parameters.

Every figure asserted on the ORACLE's side (corner counts, tracked fractions, derivative maxima) only keeps a comparison from
passing empty; none of them is a tolerance: the device result is always compared with assert_array_equal."""
import numpy as np
import pytest

from tests.test_klt_gpu import _dump
from tests.test_oracle_klt import CLAHE_PARAMS
from tests.util import binarised_image, constant_image, low_contrast_image, noise_image, shifted

pytestmark = pytest.mark.gpu

SIZES = [(416, 352), (401, 347)]      # 13 x 11 tiles of k_pyr_a, levels 208x176 / 104x88 / 52x44; odd and a multiple of no grid.  Both fused.
SEED = 21
NONE = np.zeros((0, 2))


@pytest.fixture(scope="module")
def mods():
    from oracle import klt_oracle as ko
    from xrslam_amd import klt
    return ko, klt


@pytest.fixture(scope="module")
def contexts(mods):
    """One context per (size, max_points) for the whole module."""
    _, klt = mods
    cache = {}

    def get(w, h, max_points=150):
        key = (w, h, max_points)
        if key not in cache:
            cache[key] = klt.KltContext(w, h, max_points)
        return cache[key]

    yield get
    cache.clear()


_frames = {}


def _frame(kind, w, h):
    """N: band-limited noise; B: N cut at its median to {0, 255}; L: about 15 grey levels; C<v>: constant."""
    key = (kind, w, h)
    if key not in _frames:
        if kind[0] == "C":
            g = constant_image(w, h, int(kind[1:]))
        else:
            g = {"N": noise_image, "B": binarised_image, "L": low_contrast_image}[kind](w, h, seed=SEED)
        g.setflags(write=False)
        _frames[key] = g
    return _frames[key]


def _eq(tag, got, want, **more):
    if not np.array_equal(got, want):
        _dump("params_" + "".join(ch if ch.isalnum() else "_" for ch in tag), got=got, want=want, **more)
    np.testing.assert_array_equal(got, want, err_msg=tag)


def _assert_pyramid(H, O, tag):
    """All four levels: image, derivatives, and the plane with its 21-pixel reflect-101 border."""
    for l in range(4):
        hi, hd = H.level(l)
        oi, od = O.level(l)
        op, _ = O.level(l, padded=True)
        assert hi.shape == oi.shape
        _eq("%s level %d image" % (tag, l), hi, oi)
        _eq("%s level %d derivatives" % (tag, l), hd, od)
        _eq("%s level %d padded plane" % (tag, l), H.level_padded(l), op)


def _oracle(ko, g, params=(6.0, 8, 8)):
    O = ko.OracleImage(g)
    O.preprocess(*params)
    return O


def _assert_both_pyramid_paths(ko, ctx, g, params_list, tag):
    """preprocess() with each parameter set in turn on the SAME two image objects -- one through the fused launches (where the
    size allows them), one through the five launches they replace -- against the oracle.  Consecutive sets differ, so a plane
    left over from the set before cannot pass, and the lookup table is reallocated where the tile count grows.  -> the fused image."""
    F, U = ctx.image(g), ctx.image(g)
    try:
        for params in params_list:
            O = _oracle(ko, g, params)
            t = "%s clip %g tiles %dx%d" % ((tag,) + tuple(params))
            ctx.set_fused_pyramid(1)
            F.preprocess(*params)
            ctx.set_fused_pyramid(0)
            U.preprocess(*params)
            _assert_pyramid(F, O, t + " fused")
            _assert_pyramid(U, O, t + " five-launch")
    finally:
        ctx.set_fused_pyramid(1)
    return F


def _assert_track(HA, HB, OA, OB, pts, guess, tag):
    nx_o, st_o = OA.track_keypoints(OB, pts, guess)
    nx_h, st_h = HA.track_keypoints(HB, pts, guess)
    _eq(tag + " status", st_h, st_o, nx_h=nx_h, nx_o=nx_o, pts=pts)
    _eq(tag + " positions", nx_h, nx_o, st_o=st_o, pts=pts)
    return nx_o, st_o


def _assert_lk(HA, HB, OA, OB, pts, guess, tag):
    nx_o, st_o, _ = OA.lk(OB, pts, guess)
    nx_h, st_h = HA.lk(HB, pts, guess)
    _eq(tag + " status", st_h, st_o, nx_h=nx_h, nx_o=nx_o, pts=pts, guess=guess)
    _eq(tag + " positions", nx_h, nx_o, st_o=st_o, pts=pts, guess=guess)
    return nx_o, st_o


def _assert_harris_and_detect(ko, H, O, tag, max_points=150, min_distance=20.0):
    _eq(tag + " harris", H.harris(), ko.harris_response(O.image))
    kp_o = O.detect_keypoints(NONE, max_points, min_distance)
    _eq(tag + " corners", H.detect_keypoints(NONE, max_points, min_distance), kp_o)
    return kp_o


# ------------------------------------------------------------------------------------------------ CLAHE parameter grid
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["N", "B", "L", "C0", "C255", "C110"])
def test_clahe_parameter_grid(mods, contexts, kind, size):
    """The nine (clip, tiles_x, tiles_y) sets: rectangular grids (a transposed tiles_x / tiles_y or tile width / height shows), no
    clipping, the clip count floored at 1, residuals >= 128, one tile for the frame, the 4096-tile limit with 7 x 6-pixel tiles,
    reflect-101 extensions of up to 47 pixels -- on mid-contrast, two-level, low-contrast (a dozen occupied bins) and constant
    (one bin) frames."""
    ko, _ = mods
    w, h = size
    _assert_both_pyramid_paths(ko, contexts(w, h), _frame(kind, w, h), CLAHE_PARAMS, "%s %dx%d" % (kind, w, h))


def test_clahe_grid_limits(mods, contexts):
    """More than 4096 tiles and an empty grid are refused; 4096 tiles in one row (one pixel wide each) are not."""
    ko, _ = mods
    from xrslam_amd._lib import XRHIP_EINVAL, XrhipError
    w, h = SIZES[0]
    g = _frame("N", w, h)
    ctx = contexts(w, h)
    im = ctx.image(g)
    for tx, ty in [(4097, 1), (1, 4097), (241, 17), (0, 8), (8, 0), (0, 0), (-8, 8)]:
        with pytest.raises(XrhipError) as e:
            im.preprocess(6.0, tx, ty)
        assert e.value.code == XRHIP_EINVAL, (tx, ty)
    im.preprocess(6.0, 4096, 1)
    _assert_pyramid(im, _oracle(ko, g, (6.0, 4096, 1)), "4096x1 tiles")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["N", "B"])
def test_detect_and_track_over_clahe_parameters(mods, contexts, kind, size):
    """Harris response, corners and tracks onto the frame moved by (3, -2) for the first five parameter sets.  The oracle alone finds
    106 - 113 corners in every one of them at 416 x 352 (100 - 111 at 401 x 347) and tracks at least 97 % of them on B."""
    ko, _ = mods
    w, h = size
    g = _frame(kind, w, h)
    g2 = shifted(g, 3, -2)
    ctx = contexts(w, h)
    HA, HB = ctx.image(g), ctx.image(g2)
    tracked = []
    for params in CLAHE_PARAMS[:5]:
        tag = "%s %dx%d clip %g tiles %dx%d" % ((kind, w, h) + tuple(params))
        HA.preprocess(*params)
        HB.preprocess(*params)
        OA, OB = _oracle(ko, g, params), _oracle(ko, g2, params)
        kp = _assert_harris_and_detect(ko, HA, OA, tag)
        assert len(kp) >= 80, tag
        _, st = _assert_track(HA, HB, OA, OB, kp, None, tag)
        assert st.any(), tag
        tracked.append(st.mean())
    if kind == "B":
        assert min(tracked) >= 0.97


# ------------------------------------------------------------------------------------------------------------ size edges
SIZE_EDGES = [(64, 64), (67, 65), (345, 64), (64, 345), (344, 345), (345, 345), (346, 347)]


@pytest.mark.parametrize("size", SIZE_EDGES, ids=lambda s: "%dx%d" % s)
def test_size_edges(mods, contexts, size):
    """From the smallest frame the API accepts (level 3 is 8 x 8: several reflections per border pixel) across the fused-pyramid
    switch: every level is at least 44 pixels a side from 345 on, so 344 x 345 stays on the five launches and 345 x 345 is the
    smallest fused frame (which path ran cannot be observed: the bytes on both sides of the switch are the check).  Pyramid with
    borders on both paths, Harris response, corners (the oracle finds none at 64 x 64, some tens at 345 x 345) and plain LK on 64
    points, some of them outside the frame."""
    ko, _ = mods
    w, h = size
    g = noise_image(w, h, seed=SEED)
    g2 = shifted(g, 1.5, 0.5)
    ctx = contexts(w, h)
    tag = "%dx%d" % (w, h)
    HA = _assert_both_pyramid_paths(ko, ctx, g, [(6.0, 8, 8)], tag)
    HB = ctx.image(g2)
    HB.preprocess()
    OA, OB = _oracle(ko, g), _oracle(ko, g2)
    _assert_pyramid(HB, OB, tag + " second frame")
    _assert_harris_and_detect(ko, HA, OA, tag)
    rng = np.random.RandomState(w * 1000 + h)
    pts = (rng.rand(64, 2) * [w + 48, h + 40] - [24, 20]).astype(np.float32)
    guess = (pts + [1.5, 0.5] + rng.uniform(-3, 3, (64, 2))).astype(np.float32)
    _, st = _assert_lk(HA, HB, OA, OB, pts, guess, tag + " lk")
    assert 0 < st.sum() < len(st)


# ------------------------------------------------------------------------------------------------------ extreme contrast
@pytest.mark.parametrize("params", [(0.5, 3, 5), (6.0, 8, 8)], ids=lambda p: "clip%g_%dx%d" % p)
def test_extreme_contrast(mods, contexts, params):
    """A two-level frame: level-0 Scharr derivatives of 4064 (clip 0.5, 3 x 5) and 4000 (6.0, 8 x 8) of the possible 4080, where
    the 32-bit wavefront sums of the LK template's A terms have 0.8 % of headroom, the taps are 24-bit multiplies and Harris keeps
    its Sobel values in 16 bits."""
    ko, _ = mods
    w, h = SIZES[0]
    g = _frame("B", w, h)
    g2 = shifted(g, -4, 3)
    ctx = contexts(w, h)
    tag = "B extreme clip %g tiles %dx%d" % params
    HA = _assert_both_pyramid_paths(ko, ctx, g, [params], tag)
    HB = ctx.image(g2)
    HB.preprocess(*params)
    OA, OB = _oracle(ko, g, params), _oracle(ko, g2, params)
    assert np.abs(OA.level(0)[1].astype(np.int32)).max() >= 3900
    _assert_pyramid(HB, OB, tag + " second frame")
    kp = _assert_harris_and_detect(ko, HA, OA, tag)
    assert len(kp) >= 80
    for guess in (None, kp + [-4.0, 3.0]):
        _, st = _assert_track(HA, HB, OA, OB, kp, guess, tag + (" guess" if guess is not None else ""))
        assert st.any()
    rng = np.random.RandomState(5)
    pts = (rng.rand(200, 2) * [w + 48, h + 40] - [24, 20]).astype(np.float32)   # includes points outside the frame
    guess = pts + rng.randn(200, 2).astype(np.float32) * 3
    _, st = _assert_lk(HA, HB, OA, OB, pts, guess, tag + " lk")
    assert 0 < st.sum() < len(st)


# ------------------------------------------------------------------------------------------ LK across the search tile
@pytest.fixture(scope="module")
def noise_pair(mods, contexts):
    """N at 416 x 352 with the default parameters: frame, its device and oracle images, the oracle's corners."""
    ko, _ = mods
    w, h = SIZES[0]
    g = _frame("N", w, h)
    ctx = contexts(w, h)
    HA = ctx.image(g)
    HA.preprocess()
    OA = _oracle(ko, g)
    return g, ctx, HA, OA, OA.detect_keypoints(NONE, 150, 20.0)


S40_FRACTION = {}


@pytest.mark.parametrize("s", [6, 12, 24, 40, 48])
def test_track_without_a_guess_over_growing_shifts(mods, noise_pair, s):
    """track_keypoints fetches every level's search tile round the CURRENT position when it has no guess; the frame moved by s
    pixels in +-x and +-y takes the iterations 5 + 0..3 pixels and more away from it, at level 0 first and at the coarser levels
    as s grows.  The oracle tracks 98 % at s = 6 and a fifth to two thirds at s = 48: successes and failures are both compared."""
    ko, _ = mods
    g, ctx, HA, OA, kp = noise_pair
    assert len(kp) >= 80
    HB = ctx.image()
    for dx, dy in [(s, 0), (-s, 0), (0, s), (0, -s)]:
        g2 = shifted(g, dx, dy)
        HB.upload(g2)
        HB.preprocess()
        _, st = _assert_track(HA, HB, OA, _oracle(ko, g2), kp, None, "shift (%d, %d)" % (dx, dy))
        if s == 40:
            assert 0.1 < st.mean() < 0.95, (dx, dy, st.mean())
        if s == 6:
            assert st.mean() > 0.9, (dx, dy, st.mean())


@pytest.mark.parametrize("scale", [1, 8], ids=["level0", "level3"])
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
def test_lk_guess_offsets_across_the_tile_boundary(mods, noise_pair, axis, scale):
    """Plain LK from a guess d pixels off the true position, d = +-4 .. +-9 along one axis (times 8: the same at level 3), for
    256 integer points whose x covers every residue mod 4 (the tile's left edge is moved down to a dword boundary: 0 - 3 pixels of
    slack).  The tile reaches 5 pixels round the guess, so the iteration starts inside it, on its edge and beyond it -- the
    global-memory branch -- in all four directions."""
    ko, _ = mods
    g, ctx, HA, OA, _ = noise_pair
    g2 = shifted(g, 1.5, 0.5)
    HB = ctx.image(g2)
    HB.preprocess()
    OB = _oracle(ko, g2)
    ii, jj = np.meshgrid(np.arange(16), np.arange(16))
    pts = np.stack([40 + 21 * ii.ravel(), 40 + 17 * jj.ravel()], axis=1).astype(np.float32)
    assert sorted(set(pts[:, 0].astype(int) % 4)) == [0, 1, 2, 3]
    true = pts + np.array([1.5, 0.5], np.float32)
    ok = 0
    for d in [4, 5, 6, 7, 8, 9]:
        for sign in (1, -1):
            off = np.zeros(2, np.float32)
            off[axis] = sign * d * scale
            _, st = _assert_lk(HA, HB, OA, OB, pts, true + off, "lk offset %+d along %s" % (sign * d * scale, "xy"[axis]))
            ok += int(st.sum())
    assert ok > 0


# ------------------------------------------------------------------------------------------------------- point counts
def test_track_point_counts_across_the_inline_limit(mods):
    """xrhip_image_track sends up to 160 points inline in the kernel's argument block (converted to float on the host) and more
    through pinned memory the kernel reads itself; a context made for 150 points grows its device lists past 300 points and its
    pinned block past 512.  In this order on one fresh context, with and without a guess; and the first 160 results of the
    161-point call are the 160-point call's: the two routes agree with each other."""
    ko, klt = mods
    w, h = SIZES[0]
    g = _frame("N", w, h)
    g2 = shifted(g, 3, -2)
    ctx = klt.KltContext(w, h, 150)
    HA, HB = ctx.image(g), ctx.image(g2)
    HA.preprocess()
    HB.preprocess()
    OA, OB = _oracle(ko, g), _oracle(ko, g2)
    kp = OA.detect_keypoints(NONE, 150, 20.0)
    assert len(kp) >= 80
    rng = np.random.RandomState(6)
    pts = np.concatenate([kp, rng.rand(700 - len(kp), 2) * [w - 1, h - 1]], axis=0)
    guesses = pts + [3.0, -2.0] + rng.uniform(-1, 1, pts.shape)
    res = {}
    for n in [1, 159, 160, 161, 320, 700]:
        for has in (0, 1):
            nx, st = _assert_track(HA, HB, OA, OB, pts[:n], guesses[:n] if has else None, "n = %d guess %d" % (n, has))
            res[n, has] = (nx, st)
        if n >= 159:
            assert 0 < res[n, 1][1].sum() < n
    for has in (0, 1):
        np.testing.assert_array_equal(res[161, has][0][:160], res[160, has][0])
        np.testing.assert_array_equal(res[161, has][1][:160], res[160, has][1])


# ------------------------------------------------------------------------------------------------ detection parameters
ORACLE_CORNERS_600 = {7.5: 186, 15.0: 186, 20.0: 186, 33.5: 44, 60.0: 18}     # the oracle alone, N at 416 x 352, nothing to avoid


@pytest.mark.parametrize("ctx_points", [150, 600])
def test_detection_parameters(mods, contexts, ctx_points):
    """min_distance other than the 20 of the GFTT pass (which keeps its literal 20: only the Poisson filter takes the parameter),
    one to 600 corners asked for, and points to avoid: none; 40 with some outside the frame, some exactly on the 20-pixel border
    lines and duplicates; 3000 random ones that leave room for almost nothing."""
    ko, _ = mods
    w, h = SIZES[0]
    g = _frame("N", w, h)
    ctx = contexts(w, h, ctx_points)
    H = ctx.image(g)
    H.preprocess()
    O = _oracle(ko, g)
    kp = O.detect_keypoints(NONE, 150, 20.0)
    rng = np.random.RandomState(8)
    tracked = np.concatenate([kp[:60:3] + rng.uniform(-4, 4, (20, 2)),
                              [[-5.0, 100.0], [w + 84.5, 100.0], [100.0, -3.25], [100.0, h + 48.0], [-40.0, -40.0], [w + 0.0, h + 0.0]],
                              [[20.0, 100.0], [w - 20.0, 200.0], [150.0, 20.0], [250.0, h - 20.0], [20.0, 20.0], [w - 20.0, h - 20.0]],
                              kp[60:66], kp[60:62]], axis=0)
    assert len(tracked) == 40
    crowd = rng.rand(3000, 2) * [w, h]
    admitted = {}
    for name, have in (("none", NONE), ("tracked", tracked), ("crowd", crowd)):
        for md in [7.5, 15.0, 20.0, 33.5, 60.0]:
            for mp in [1, 5, 150, 600]:
                want = O.detect_keypoints(have, mp, md)
                _eq("detect %s min_distance %g max_points %d" % (name, md, mp), H.detect_keypoints(have, mp, md), want)
                admitted[name, md, mp] = len(want) - len(have)
    for md, n in ORACLE_CORNERS_600.items():
        assert admitted["none", md, 600] == n, (md, admitted["none", md, 600])
    assert admitted["none", 20.0, 1] <= 1 and 0 < admitted["none", 20.0, 5] <= 5      # (the strongest corner lies in the 20-pixel border)
    assert 0 < admitted["tracked", 20.0, 150] < admitted["none", 20.0, 150]
    assert admitted["crowd", 60.0, 600] == 0 and admitted["crowd", 7.5, 600] < 40
