"""tests/scale_model.py checked against itself (by hand, and through the properties the other frame-scaling tests rest on), and
XRSLAMAmdScaleIntrinsics against the model's coordinate map.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import scale_model as sm


def _noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w), dtype=np.uint8)


def test_three_to_two_by_hand():
    """cw = 3 -> W = 2: units of 1/2 source pixel; working pixel 0 spans [0, 3) = all of column 0 (2) and half of column 1 (1),
    working pixel 1 the other half (1) and column 2 (2)."""
    np.testing.assert_array_equal(sm.weights(2, 3), [[2, 1, 0], [0, 1, 2]])
    row = np.array([[10, 40, 250]], np.uint8)
    #  (2*10 + 40 + 1) // 3 = 20      (40 + 2*250 + 1) // 3 = 180
    np.testing.assert_array_equal(sm.scale_gray(row, (3, 1, 0, 0, 3, 1), 2, 1), [[20, 180]])
    # the same vertically, and both at once: (2*2*10 + 2*40 + 2*20 + 80 + 4) // 9 = 27
    np.testing.assert_array_equal(sm.scale_gray(row.T.copy(), (1, 3, 0, 0, 1, 3), 1, 2), [[20], [180]])
    g = np.array([[10, 40, 0], [20, 80, 0], [0, 0, 0]], np.uint8)
    assert sm.scale_gray(g, (3, 3, 0, 0, 3, 3), 2, 2)[0, 0] == (4 * 10 + 2 * 40 + 2 * 20 + 80 + 4) // 9 == 27


def test_ratio_one_is_a_crop():
    g = _noise(40, 30, 1)
    np.testing.assert_array_equal(sm.scale_gray(g, (40, 30, 7, 5, 21, 18), 21, 18), g[5:23, 7:28])
    np.testing.assert_array_equal(sm.scale_gray(g, (40, 30, 0, 0, 40, 30), 40, 30), g)


@pytest.mark.parametrize("kx,ky", [(2, 2), (3, 3), (3, 2), (2, 1)])
def test_replicated_pixels_scale_back_to_the_original_bits(kx, ky):
    g = _noise(33, 21, 2)
    big = sm.replicate(g, kx, ky)
    assert big.shape == (21 * ky, 33 * kx)
    np.testing.assert_array_equal(sm.scale_gray(big, (33 * kx, 21 * ky, 0, 0, 33 * kx, 21 * ky), 33, 21), g)
    # ... inside a larger frame too
    frame = _noise(33 * kx + 9, 21 * ky + 4, 3)
    frame[3:3 + 21 * ky, 5:5 + 33 * kx] = big
    np.testing.assert_array_equal(sm.scale_gray(frame, (33 * kx + 9, 21 * ky + 4, 5, 3, 33 * kx, 21 * ky), 33, 21), g)


def test_integer_ratio_is_the_box_mean():
    g = _noise(24, 18, 4)
    want = (g.astype(np.int64).reshape(6, 3, 8, 3).sum((1, 3)) * 2 + 9) // 18   # (sum + 4.5) / 9, floored
    np.testing.assert_array_equal(sm.scale_gray(g, (24, 18, 0, 0, 24, 18), 8, 6), want)


@pytest.mark.parametrize("v", [0, 1, 127, 254, 255])
def test_a_constant_image_stays_constant_for_coprime_ratios(v):
    for (cw, ch), (W, H) in (((131, 101), (97, 66)), ((17, 13), (5, 4)), ((1692, 7), (752, 3))):
        g = np.full((ch, cw), v, np.uint8)
        np.testing.assert_array_equal(sm.scale_gray(g, (cw, ch, 0, 0, cw, ch), W, H), np.full((H, W), v))


def test_rounds_half_up_at_an_exact_tie():
    geo = (2, 2, 0, 0, 2, 2)
    for block, want in (([[0, 0], [0, 2]], 1), ([[0, 0], [1, 1]], 1), ([[0, 0], [0, 1]], 0), ([[255, 255], [255, 254]], 255),
                        ([[1, 0], [0, 0]], 0), ([[1, 1], [1, 0]], 1)):
        assert sm.scale_gray(np.array(block, np.uint8), geo, 1, 1)[0, 0] == want, block


def test_formats_are_reduced_per_source_pixel_before_averaging():
    from tests import pixfmt_model as pm
    # limited range: 16 -> 0 and 235 -> 255, mean 128 (127.5 rounded up); averaging first would give expand(125.5) = 127 or 128 by luck,
    # so use a pair where the orders differ: 0 and 32 -> 0 and 19 -> 10 (9.5 up); mean first: expand(16) = 0
    px = np.array([[[0], [32]]], np.uint8)
    assert sm.scale(px, (2, 1, 0, 0, 2, 1), 1, 1, pm.GRAY8, 0, 1)[0, 0] == 10
    # GRAY16, 10 bits: samples 1023 and 2047 -> 255 and 255 (clamped per pixel)
    px = pm.samples16(np.array([[1023, 2047]]))
    assert sm.scale(px, (2, 1, 0, 0, 2, 1), 1, 1, pm.GRAY16, 10)[0, 0] == 255


def test_scale_intrinsics_maps_the_principal_point_and_a_crop_corner_like_the_model():
    from xrslam_amd import _lib
    from xrslam_amd.harness import runner
    lib = runner.load(_lib.LIB_PATH)
    W, H = 752, 480
    for geo, K in (((1920, 1080, 114, 0, 1692, 1080), (1400.5, 1399.25, 961.75, 538.5)),
                   ((1280, 720, 33, 17, 1001, 653), (900.0, 905.0, 640.0, 360.0)),
                   ((752, 480, 0, 0, 752, 480), (458.654, 457.296, 367.215, 248.375))):
        src = np.array(K, np.float64)
        out = np.zeros(4)
        lib.XRSLAMAmdScaleIntrinsics(src.ctypes.data, C.byref(runner.frame_geometry(geo)), W, H, out.ctypes.data)
        np.testing.assert_allclose(out, sm.scale_intrinsics(K, geo, W, H), rtol=0, atol=1e-12)
        fx, fy, cx, cy = out
        # the principal point: the ray (0, 0, 1) lands on (cx, cy) of the source, and on the model's image of that point
        np.testing.assert_allclose((cx, cy), sm.map_point(K[2], K[3], geo, W, H), rtol=0, atol=1e-9)
        # the crop's outer corners: source coordinates crop_x - 0.5 / crop_x + cw - 0.5 are the working image's -0.5 / W - 0.5
        _, _, x0, y0, cw, ch = geo
        for u, v, wu, wv in ((x0 - 0.5, y0 - 0.5, -0.5, -0.5), (x0 + cw - 0.5, y0 + ch - 0.5, W - 0.5, H - 0.5)):
            ray = ((u - K[2]) / K[0], (v - K[3]) / K[1])
            np.testing.assert_allclose((fx * ray[0] + cx, fy * ray[1] + cy), (wu, wv), rtol=0, atol=1e-9)
            np.testing.assert_allclose(sm.map_point(u, v, geo, W, H), (wu, wv), rtol=0, atol=1e-9)
    np.testing.assert_allclose(out, src, rtol=0, atol=1e-12)   # (the last one: the identity geometry changes nothing)
