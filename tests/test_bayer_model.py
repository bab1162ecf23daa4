"""The Bayer model (tests/bayer_model.py) against values that follow from the definition by hand."""
import numpy as np
import pytest

from tests import bayer_model as bm
from tests import scale_model as sm


def _random(w, h, fmt, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, bm.BYTES[fmt]), dtype=np.uint8)


@pytest.mark.parametrize("fmt", bm.FORMATS, ids=[bm.NAMES[f] for f in bm.FORMATS])
def test_a_constant_mosaic_gives_the_constant(fmt):
    """The weights sum to 16384 and every sum is four times a mean of equal samples: v comes out, borders included."""
    for v in (0, 1, 77, 128, 254, 255):
        if bm.BYTES[fmt] == 1:
            px = np.full((6, 7, 1), v, np.uint8)
            got = bm.reduce(px, fmt)
        else:   # 12 significant bits: v in bits 4..11, anything below
            px = np.zeros((6, 7, 2), np.uint8)
            px[..., 0] = ((v << 4) & 255) | 9
            px[..., 1] = v >> 4
            got = bm.reduce(px, fmt, 12)
        np.testing.assert_array_equal(got, np.full((6, 7), v, np.uint8))


@pytest.mark.parametrize("colour,want", [("red", 76), ("green", 150), ("blue", 29)])
def test_one_lit_colour_gives_its_weight(colour, want):
    """Only the sites of one colour hold 255: the bilinear estimate of that channel is 255 at every pixel (four times it: 1020) and
    the others are 0, so gray = (weight * 1020 + 32768) >> 16: red 4899 -> 76, green 9617 -> 150, blue 1868 -> 29.  (The mirrored
    border keeps every neighbour on its colour, so this holds at the border too; the interior is what is asserted.)"""
    assert [(wgt * 1020 + 32768) >> 16 for wgt in (4899, 9617, 1868)] == [76, 150, 29]
    for fmt in bm.FORMATS[:4]:
        red, g_red, g_blue, blue = bm.sites(9, 10, bm.PHASE[fmt])
        lit = {"red": red, "green": g_red | g_blue, "blue": blue}[colour]
        got = bm.reduce(np.where(lit, 255, 0).astype(np.uint8)[..., None], fmt)
        np.testing.assert_array_equal(got[1:-1, 1:-1], np.full((7, 8), want, np.uint8), err_msg=bm.NAMES[fmt])
        np.testing.assert_array_equal(got, np.full((9, 10), want, np.uint8), err_msg=bm.NAMES[fmt] + ", border")


@pytest.mark.parametrize("fmt", [bm.GRBG8, bm.GBRG8, bm.BGGR8, bm.GRBG16, bm.GBRG16, bm.BGGR16], ids=lambda f: bm.NAMES[f])
def test_a_pattern_is_rggb_on_the_frame_shifted_by_its_phase(fmt):
    """The frame without its first px columns and py rows, read as the pattern with phase (px, py), has every sample on the site it
    had in the RGGB frame: the interior pixels (whose neighbours are the same samples) come out the same."""
    px, py = bm.PHASE[fmt]
    rggb = bm.RGGB8 if bm.BYTES[fmt] == 1 else bm.RGGB16
    big = _random(23, 18, fmt, seed=fmt)
    whole = bm.reduce(big, rggb)
    part = bm.reduce(np.ascontiguousarray(big[py:, px:]), fmt)
    np.testing.assert_array_equal(part[1:-1, 1:-1], whole[py:, px:][1:-1, 1:-1])
    assert (part != bm.reduce(np.ascontiguousarray(big[py:, px:]), rggb)).mean() > 0.5     # and the phase does matter


def test_the_mirrored_border_by_hand():
    """RGGB, s(x, y) = 10 (1 + x + 4 y).  Worked from the definition:
      (0,0) red:    C = 40;  P = 20 + 20 + 50 + 50 = 140;  X = 4 * 60 = 240         (195960 + 1346380 + 448320 + 32768) >> 16 = 30
      (3,0) green between reds:  C = 160;  Hh = 2 (30 + 30) = 120;  Vv = 2 (80 + 80) = 320         R4 = Hh, B4 = Vv -> 42
      (0,2) red:    C = 360;  P = 100 + 100 + 50 + 130 = 380;  X = 2 * 60 + 2 * 140 = 400          -> 94
      (0,3) green between blues: C = 520;  Hh = 2 (140 + 140) = 560;  Vv = 2 (90 + 90) = 360       R4 = Vv, B4 = Hh -> 119
      (3,3) blue:   C = 640;  P = 150 + 150 + 120 + 120 = 540;  X = 4 * 110 = 440                  R4 = X -> 130
      (1,1) blue, interior: C = P = X = 240                                                        -> (240 * 16384 + 32768) >> 16 = 60"""
    s = (10 * (1 + np.arange(4)[None, :] + 4 * np.arange(4)[:, None])).astype(np.uint8)
    got = bm.reduce(s[..., None], bm.RGGB8)
    assert (4899 * 40 + 9617 * 140 + 1868 * 240 + 32768) >> 16 == 30
    assert (4899 * 120 + 9617 * 160 + 1868 * 320 + 32768) >> 16 == 42
    assert (4899 * 360 + 9617 * 380 + 1868 * 400 + 32768) >> 16 == 94
    assert (4899 * 360 + 9617 * 520 + 1868 * 560 + 32768) >> 16 == 119
    assert (4899 * 440 + 9617 * 540 + 1868 * 640 + 32768) >> 16 == 130
    assert [got[0, 0], got[0, 3], got[2, 0], got[3, 0], got[3, 3], got[1, 1]] == [30, 42, 94, 119, 130, 60]
    # the same samples as 16-bit values with 8 significant bits and a set bit above them: saturated to 255 first
    px16 = np.stack([s, np.zeros_like(s)], -1)
    np.testing.assert_array_equal(bm.reduce(px16, bm.RGGB16, 8), got)
    px16[..., 1] = 1
    np.testing.assert_array_equal(bm.reduce(px16, bm.RGGB16, 8), np.full((4, 4), 255, np.uint8))


def test_the_scaled_composition_demosaics_the_crop_as_a_frame_of_its_own():
    """An odd crop origin shifts the phase: the crop of a GRBG frame at (3, 5) is a frame of its own with phase
    ((1 + 3) & 1, (0 + 5) & 1) = (0, 1): GBRG.  A crop of the plane's size is that frame's gray plane; a 2x crop its 2 x 2 box mean."""
    W, H = 32, 32
    big = _random(70, 67, bm.GRBG8, seed=5)
    geo = (70, 67, 3, 5, 32, 32)
    np.testing.assert_array_equal(bm.scale(big, geo, W, H, bm.GRBG8), bm.reduce(np.ascontiguousarray(big[5:37, 3:35]), bm.GBRG8))
    geo = (70, 67, 2, 0, 64, 64)
    g = bm.reduce(np.ascontiguousarray(big[0:64, 2:66]), bm.GRBG8).astype(np.int64)
    box = (g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) // 4
    np.testing.assert_array_equal(bm.scale(big, geo, W, H, bm.GRBG8), box)
    assert sm.MAX_AREA == 1 << 24
