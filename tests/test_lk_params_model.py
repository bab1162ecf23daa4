"""CPU: tests/lk_params_model.py at the reference's parameters IS orc_track_keypoints -- positions and status, bit for bit."""
import numpy as np
import pytest

from tests import lk_params_model as lm
from tests.util import noise_image, shifted


@pytest.mark.parametrize("size,shift", [((416, 352), (3, -2)), ((401, 347), (-14, 9)), ((416, 352), (40, 0))],
                         ids=["small_shift", "odd_size", "large_shift"])
@pytest.mark.parametrize("with_guess", [False, True], ids=["no_guess", "guess"])
def test_model_equals_orc_track_keypoints_at_the_reference_parameters(size, shift, with_guess):
    from oracle import klt_oracle as ko
    w, h = size
    g = noise_image(w, h, seed=21)
    g2 = shifted(g, *shift)
    OA, OB = ko.OracleImage(g), ko.OracleImage(g2)
    OA.preprocess()
    OB.preprocess()
    kp = OA.detect_keypoints(np.zeros((0, 2)), 150, 20.0)
    assert len(kp) >= 80
    rng = np.random.RandomState(3)
    # corners, points anywhere in and round the frame (border gate, templates outside), sub-pixel positions
    pts = np.concatenate([kp, rng.rand(200, 2) * [w + 48, h + 40] - [24, 20]], axis=0)
    guess = pts + np.array(shift, np.float64) + rng.uniform(-2, 2, pts.shape) if with_guess else None
    nx_o, st_o = OA.track_keypoints(OB, pts, guess)
    nx_m, st_m = lm.track_keypoints(OA, OB, pts, guess, 21, 3, 30, 0.01)
    assert 0 < st_o.sum() < len(st_o)            # successes and failures are both compared
    np.testing.assert_array_equal(st_m, st_o)
    np.testing.assert_array_equal(nx_m, nx_o)


def test_deeper_oracle_pyramid_extends_the_default_one():
    """The first four levels of a six-level oracle pyramid are the four-level pyramid's, borders included."""
    from oracle import klt_oracle as ko
    g = noise_image(416, 352, seed=21)
    O3 = ko.OracleImage(g)
    O3.preprocess()
    O5 = lm.oracle_image(g, 5)
    for l in range(4):
        for a, b in zip(O3.level(l, padded=True), O5.level(l, padded=True)):
            np.testing.assert_array_equal(a, b)
    assert O5.level(5)[0].shape == (11, 13)
