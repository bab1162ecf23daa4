"""tests/mask_model.py against the CPU oracle: with an all-ones mask the model IS OpenCvImage::detect_keypoints (oracle/klt_oracle.c),
key point for key point and in order -- which is what entitles it to stand in for the oracle where a mask is present
(tests/test_mask_gpu.py).  Then the properties the mask adds."""
import os

import numpy as np
import pytest

from oracle import klt_oracle as ko
from tests import mask_model as mm
from tests.util import noise_image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "euroc_pair.npz")


def existing_points(w, h, n, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(15, w - 15, n), rs.uniform(15, h - 15, n)], axis=1)


def frames():
    return {"euroc": np.load(GOLDEN)["a"], "noise_320": noise_image(320, 240, seed=5), "noise_200": noise_image(200, 136, seed=9)}


@pytest.fixture(scope="module")
def planes():
    """name -> (the CLAHE image the oracle detects on, its Harris response)"""
    out = {}
    for name, g in frames().items():
        o = ko.OracleImage(g)
        o.preprocess()
        out[name] = (o, ko.harris_response(o.image))
    return out


@pytest.mark.parametrize("name", ["euroc", "noise_320", "noise_200"])
@pytest.mark.parametrize("n_exist", [0, 40])
@pytest.mark.parametrize("max_points", [150, 20])
def test_all_ones_mask_is_the_oracle(planes, name, n_exist, max_points):
    o, resp = planes[name]
    ex = existing_points(o.w, o.h, n_exist, seed=3)
    want = o.detect_keypoints(ex, max_points, 20.0)[n_exist:]
    got = mm.detect(resp, np.ones(resp.shape, np.uint8), ex, max_points, 20.0)
    assert len(want) > 0 or n_exist   # (existing points may leave a small frame no room)
    assert np.array_equal(got, want)


def one_strong_corner(w=320, h=240):
    """Low-contrast texture with one high-contrast checker corner: the corner's response sets a threshold that most of the texture's
    corners do not reach."""
    g = (110.0 + (noise_image(w, h, seed=21).astype(np.float64) - 110.0) * 0.12).round().astype(np.uint8)
    cy, cx = 100, 100
    g[cy - 12:cy, cx - 12:cx] = 250
    g[cy:cy + 12, cx:cx + 12] = 250
    g[cy - 12:cy, cx:cx + 12] = 5
    g[cy:cy + 12, cx - 12:cx] = 5
    return g


def test_hiding_the_global_maximum_lowers_the_threshold():
    """Rule 2: the maximum is taken over visible pixels.  A post-filter of the unmasked candidate list keeps the old threshold."""
    resp = ko.harris_response(one_strong_corner())
    h, w = resp.shape
    ones = np.ones((h, w), np.uint8)
    my, mx = np.unravel_index(np.argmax(resp), resp.shape)
    mask = ones.copy()
    mask[max(my - 30, 0):my + 31, max(mx - 30, 0):mx + 31] = 0
    assert mm.threshold(resp, mask) < mm.threshold(resp, ones)
    idx_all, _ = mm.candidates(resp, ones)
    post = [i for i in idx_all if mask.reshape(-1)[i]]
    idx_m, _ = mm.candidates(resp, mask)
    assert len(idx_m) > len(post)
    assert set(post) <= set(idx_m.tolist())


@pytest.mark.parametrize("kind", ["left_half", "checker", "rect"])
def test_no_point_on_a_zero_byte(planes, kind):
    o, resp = planes["noise_320"]
    h, w = resp.shape
    mask = np.ones((h, w), np.uint8)
    if kind == "left_half":
        mask[:, :w // 2] = 0
    elif kind == "checker":
        mask[(np.add.outer(np.arange(h), np.arange(w)) & 1) == 0] = 0
    else:
        mask[60:180, 80:240] = 0
    for ex in (np.zeros((0, 2)), existing_points(w, h, 30, seed=4)):
        pts = mm.detect(resp, mask, ex, 150, 20.0)
        assert len(pts) > 0
        assert not mm.on_zero_byte(pts, mask).any()
    cand, _ = mm.candidates(resp, mask)
    assert mask.reshape(-1)[cand].all()


def test_nonzero_values_are_equivalent(planes):
    o, resp = planes["noise_200"]
    rs = np.random.RandomState(1)
    base = rs.randint(0, 2, size=resp.shape).astype(np.uint8)
    a = mm.detect(resp, base, np.zeros((0, 2)), 150, 20.0)
    b = mm.detect(resp, base * rs.choice([1, 128, 255], size=resp.shape).astype(np.uint8), np.zeros((0, 2)), 150, 20.0)
    assert np.array_equal(a, b)


def test_all_zero_mask_returns_nothing(planes):
    o, resp = planes["noise_320"]
    zero = np.zeros(resp.shape, np.uint8)
    assert mm.masked_max(resp, zero) is None
    assert len(mm.candidates(resp, zero)[0]) == 0
    assert mm.detect(resp, zero, existing_points(320, 240, 10, seed=2), 150, 20.0).shape == (0, 2)


def test_track_gate():
    mask = np.ones((40, 60), np.uint8)
    mask[:, 30:] = 0
    xy = np.array([[29.49, 10.0], [29.5, 10.0], [10.0, 10.0], [45.0, 20.0], [45.0, 20.0]])
    st = np.array([1, 1, 1, 1, 0], np.uint8)
    assert mm.track_gate(xy, st, mask).tolist() == [1, 0, 1, 0, 0]
    assert st.tolist() == [1, 1, 1, 1, 0]
