"""The optional feature_tracker.lk_* keys through the outer C API on the short 320 x 240 synthetic stream of the other stream tests.
(a) the four keys written at the reference's values: the output log (tests/outlog.py) is byte-identical to the run without them.
(b) lk_window_size 15, lk_max_level 2: initialises, tracks to the end, XRSLAMAmdGetTrackerParams reports the values, the KLT
    statistics show the three-level kernels ran, and the trajectory error against the stream's ground truth stays within the margin
    of the default run's (profiles/lk_params.md has the measured figures and the reasoning)."""
import os
import tempfile

import pytest

from tests import lk_params_yaml as ly
from tests.test_color_stream_gpu import N, _parse   # N: leaves initialisation, fills the window, marginalises (asserted below)
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

W, H = 320, 240
# Measured on an MI355X on this stream (profiles/lk_params.md): ATE RMSE 0.0189 m at the default parameters, 0.0147 m at 15 / 2.  Another
# window tracks the same corners to other sub-pixel positions and loses other ones, so the two errors differ by some millimetres in
# either direction; both are the accuracy of a healthy 120-frame run, one to two centimetres.  A tracker that loses its points does
# not initialise (no poses: NaN) or drifts by decimetres on this metre-sized figure-eight.  Margin: the non-default run may have at
# most twice the default run's error plus 2 cm (0.058 m with the figures above: four times what was measured, a fifth of a decimetre
# drift).
ATE_FACTOR, ATE_SLACK = 2.0, 0.02


@pytest.fixture(scope="module")
def seq():
    return scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))


def _run(seq, slam):
    from xrslam_amd import _lib
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        s = runner.Session(_lib.LIB_PATH, seq, slam_yaml=slam, sensor_yaml=ly.SENSOR_320, instance=True)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    s.set_profiling(True)
    params = ly.tracker_params(s)
    while s.step():
        assert not s.error(), s.error()
    s.flush()
    s.sync()
    assert not s.error(), s.error()
    t = s.times()
    st = s.klt_stats()
    out = dict(params=params, counts=(t.frames, t.solves, t.solve_iterations, t.marginalizations, t.keyframes),
               ate=runner.ate_rmse(s.poses, seq), poses=len([p for p in s.poses if p[0] > 0]),
               klt=(st.n_track, st.lk_points, st.lk_templates, st.lk_iterations))
    s.close()
    with open(path, "rb") as fh:
        out["log"] = fh.read()
    os.unlink(path)
    return out


@pytest.fixture(scope="module")
def default_run(seq):
    r = _run(seq, ly.BENCH_YAML)
    F, B = _parse(r["log"])
    assert r["counts"][0] == N == len(F)
    assert len(B) >= N - 70 and r["counts"][3] >= 1 and r["counts"][4] >= 10, r["counts"]   # tracking, marginalisations, keyframes
    assert r["params"] == (21, 3, 30, 0.01)
    return r


def test_keys_at_the_reference_values_write_the_log_of_no_keys(tmp_path, seq, default_run):
    r = _run(seq, ly.slam_yaml(tmp_path / "keys.yaml", lk_window_size=21, lk_max_level=3, lk_max_iterations=30, lk_epsilon=0.01))
    assert r["params"] == (21, 3, 30, 0.01)
    assert r["counts"] == default_run["counts"] and r["klt"] == default_run["klt"]
    assert r["log"] == default_run["log"], "the output log differs from the run without the keys"


def test_window_15_level_2_tracks_the_stream(tmp_path, seq, default_run):
    r = _run(seq, ly.slam_yaml(tmp_path / "w15l2.yaml", lk_window_size=15, lk_max_level=2))
    assert r["params"] == (15, 2, 30, 0.01)
    F, B = _parse(r["log"])
    assert r["counts"][0] == N == len(F)
    assert len(B) >= N - 70 and r["counts"][3] >= 1 and r["counts"][4] >= 10, r["counts"]   # initialised, tracked to the end
    # three levels, two directions: at most 6 templates per point submitted; the four-level kernels extract 8 for every point that
    # passes the forward gates (the default run: well above 6 per point)
    n_track, points, templates, iterations = r["klt"]
    d_track, d_points, d_templates, _ = default_run["klt"]
    assert n_track > 0 and points > 0 and iterations > 0
    assert templates <= 6 * points and d_templates > 6 * d_points, (r["klt"], default_run["klt"])
    print("ATE default %.4f m, window 15 / level 2 %.4f m" % (default_run["ate"], r["ate"]))
    assert default_run["ate"] == default_run["ate"] and r["ate"] == r["ate"]              # (not NaN: both runs answered poses)
    assert r["ate"] <= ATE_FACTOR * default_run["ate"] + ATE_SLACK, (r["ate"], default_run["ate"])
