"""tests/orient_model.py checked against itself -- the index form against numpy's own mirror and quarter turn, the inverse, the
coordinate map, the intrinsics -- and the properties the other orientation tests rest on: exact area scaling commutes with all eight
orientations, so an implementation may scale in the source's orientation and turn the working-size result.  Plain numpy, no library,
no GPU."""
import numpy as np
import pytest

from tests import orient_model as om
from tests import scale_model as sm
from tests.test_scale_gpu import PLANES, geometries

ORIENTATIONS = tuple(range(8))


def _noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w), dtype=np.uint8)


def test_a_quarter_turn_clockwise_by_hand():
    g = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)          # cw = 3, ch = 2
    np.testing.assert_array_equal(om.orient(g, 1), [[4, 1], [5, 2], [6, 3]])   # the left column becomes the top row, bottom first
    np.testing.assert_array_equal(om.orient(g, 2), [[6, 5, 4], [3, 2, 1]])
    np.testing.assert_array_equal(om.orient(g, 3), [[3, 6], [2, 5], [1, 4]])
    np.testing.assert_array_equal(om.orient(g, 4), [[3, 2, 1], [6, 5, 4]])
    np.testing.assert_array_equal(om.orient(g, 5), [[6, 3], [5, 2], [4, 1]])   # mirrored, then a quarter turn clockwise
    np.testing.assert_array_equal(om.orient(g, 6), [[4, 5, 6], [1, 2, 3]])   # upside down without the mirror image
    np.testing.assert_array_equal(om.orient(g, 7), g.T)


@pytest.mark.parametrize("w,h", [(7, 5), (4, 4), (1, 6), (33, 32)])
def test_the_two_forms_agree_and_the_eight_maps_are_distinct(w, h):
    g = np.arange(w * h, dtype=np.int64).reshape(h, w)       # every pixel its own value
    outs = []
    for o in ORIENTATIONS:
        a = om.orient(g, o)
        np.testing.assert_array_equal(a, om.orient_rot90(g, o), err_msg=str(o))
        assert a.shape == om.turned_size(w, h, o)[::-1]
        outs.append(a)
    if w > 1 and h > 1:
        for i in range(8):
            for j in range(i + 1, 8):
                assert outs[i].shape != outs[j].shape or not np.array_equal(outs[i], outs[j]), (i, j)
    # a stack of frames turns frame by frame
    stack = np.stack([g, g[::-1]])
    for o in ORIENTATIONS:
        np.testing.assert_array_equal(om.orient(stack, o)[1], om.orient(g[::-1], o))


def test_the_inverse_undoes_every_orientation():
    g = _noise(13, 9, 1)
    for o in ORIENTATIONS:
        inv = om.inverse(o)
        np.testing.assert_array_equal(om.orient(om.orient(g, o), inv), g, err_msg=str(o))
        np.testing.assert_array_equal(om.orient(om.orient(g, inv), o), g, err_msg=str(o))
        assert om.inverse(inv) == o
    assert [om.inverse(o) for o in ORIENTATIONS] == [0, 3, 2, 1, 4, 5, 6, 7]


def test_a_one_hot_image_lands_where_map_point_says():
    cw, ch = 7, 5
    for o in ORIENTATIONS:
        for i, j in ((0, 0), (6, 0), (0, 4), (6, 4), (2, 3), (5, 1)):
            g = np.zeros((ch, cw), np.uint8)
            g[j, i] = 1
            u = om.orient(g, o)
            X, Y = om.map_point(i, j, o, cw, ch)
            assert u[Y, X] == 1 and u.sum() == 1, (o, i, j)


def test_orient_intrinsics_reprojects_points_like_the_coordinate_map():
    """A source pixel (u, v) is the ray ((u - cx) / fx, (v - cy) / fy, 1); R takes it to the working camera, whose intrinsics put it
    where the coordinate map puts the pixel -- for the whole frame and through crops, for every orientation."""
    W, H = 752, 480
    K = (458.654, 457.296, 367.215, 248.375)
    for geo in (None, (1920, 1080, 114, 0, 1692, 1080), (1300, 1000, 3, 5, 1111, 977)):
        for o in ORIENTATIONS:
            (fx, fy, cx, cy), R = om.orient_intrinsics(K, geo, o, W, H)
            assert fx > 0 and fy > 0
            np.testing.assert_allclose(R @ R.T, np.eye(3), atol=0)
            assert round(np.linalg.det(R)) == (-1 if o >> 2 else 1)
            x0, y0, cw, ch = om.source_geometry(geo, o, W, H)
            for u, v in ((K[2], K[3]), (x0 - 0.5, y0 - 0.5), (x0 + cw - 0.5, y0 + ch - 0.5), (x0 + 10.25, y0 + 300.5)):
                ray = R @ np.array([(u - K[2]) / K[0], (v - K[3]) / K[1], 1.0])
                assert ray[2] == 1.0
                np.testing.assert_allclose((fx * ray[0] + cx, fy * ray[1] + cy), om.map_frame_point(u, v, geo, o, W, H), rtol=0, atol=1e-9)
            # the crop's outer corners are the working image's outer corners, whichever way round
            corners = {tuple(np.round(om.map_frame_point(u, v, geo, o, W, H), 9)) for u in (x0 - 0.5, x0 + cw - 0.5)
                       for v in (y0 - 0.5, y0 + ch - 0.5)}
            assert corners == {(-0.5, -0.5), (W - 0.5, -0.5), (-0.5, H - 0.5), (W - 0.5, H - 0.5)}
    # orientation 0 is XRSLAMAmdScaleIntrinsics
    geo = (1920, 1080, 114, 0, 1692, 1080)
    np.testing.assert_allclose(om.orient_intrinsics(K, geo, 0, W, H)[0], sm.scale_intrinsics(K, geo, W, H), rtol=0, atol=1e-12)


@pytest.mark.parametrize("W,H", PLANES)
def test_exact_area_scaling_commutes_with_the_orientations(W, H):
    """orient(scale(g)) == scale(orient(g)) over the geometries of tests/test_scale_gpu.py, where the crop covers the turned plane:
    the weights of scale_model.weights are symmetric under reversal."""
    for o in ORIENTATIONS:
        pw, ph = om.turned_size(W, H, o)                       # the plane in the source's orientation
        for k, (name, geo) in enumerate(geometries(pw, ph).items()):
            sw, sh, x, y, cw, ch = geo
            g = _noise(sw, sh, 10 * o + k)
            crop = g[y:y + ch, x:x + cw]
            u = om.orient(crop, o)
            th, tw = u.shape
            by_definition = sm.scale_gray(u, (tw, th, 0, 0, tw, th), W, H)
            np.testing.assert_array_equal(om.orient(sm.scale_gray(g, geo, pw, ph), o), by_definition, err_msg="%s, o %d" % (name, o))
    for n_out, n_in in ((97, 131), (66, 101), (5, 17)):
        np.testing.assert_array_equal(sm.weights(n_out, n_in), sm.weights(n_out, n_in)[::-1, ::-1])


def test_the_exif_table():
    assert {e: om.from_exif(e) for e in range(1, 9)} == {1: 0, 6: 1, 3: 2, 8: 3, 2: 4, 7: 5, 4: 6, 5: 7}
    assert [om.from_exif(e) for e in (0, 9, -1, 100)] == [-1] * 4
    # what the tag says: 6 = "the 0th row is the visual right-hand side": a quarter turn clockwise shows it upright; 2 = mirrored
    g = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    np.testing.assert_array_equal(om.orient(g, om.from_exif(6)), np.rot90(g, -1))
    np.testing.assert_array_equal(om.orient(g, om.from_exif(2)), g[:, ::-1])
    np.testing.assert_array_equal(om.orient(g, om.from_exif(4)), g[::-1])
    np.testing.assert_array_equal(om.orient(g, om.from_exif(5)), g.T)
    np.testing.assert_array_equal(om.orient(g, om.from_exif(7)), g[::-1, ::-1].T)
