"""Turned and mirrored frames through the outer C API (include/XRSLAM.h: XRSLAMAmdSetFrameOrientation) on the short 320x240 synthetic
stream of tests/test_scale_stream_gpu.py.

A frame turned by the inverse orientation and pushed with the orientation set arrives as the original gray plane (tests/orient_model.py),
so everything behind the plane is the same: such a run must write the BYTE-identical output log (tests/outlog.py) of the plain run --
for a reversing (6: upside down) and a transposing (1: a quarter turn) orientation, inline and pipelined, from host memory and from
HBM, pushed frame by frame and through the replay loop, alone and as a member of an instance group whose other members push plain
frames."""
import os
import tempfile
import threading

import numpy as np
import pytest

from tests import color_frames as cf
from tests import orient_model as om
from tests.test_color_stream_gpu import N, _finish, _parse   # N: leaves initialisation, fills the window, marginalises (asserted below)
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR_YAML = os.path.join(ROOT, "tests", "golden", "small_sensor_320.yaml")
W, H = 320, 240
REVERSING, TRANSPOSING, MIRRORED = 6, 1, 4


@pytest.fixture(scope="module")
def seq():
    q = scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))
    g = q["frames"]
    out = dict(q, gray=g)
    for o in (REVERSING, TRANSPOSING, MIRRORED):
        turned = runner.turn_frames(g, runner.inverse_orientation(o))   # what a camera mounted that way delivers
        np.testing.assert_array_equal(turned, om.orient(g, om.inverse(o)))
        np.testing.assert_array_equal(om.orient(turned, o), g)
        assert turned.shape[1:] == om.turned_size(W, H, o)[::-1]
        out[o] = turned
    return out


@pytest.fixture(scope="module")
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


def _logged(seq, o=0, how="step", in_hbm=False, mode=0, group=None, instance=False, hbm=None):
    """One session over the frames turned for orientation o (0: the plain frames).  Host frames are turned by the session itself
    (runner.Session(orientation=)); frames in HBM are staged already turned."""
    from xrslam_amd import _lib
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    frames = seq[o] if o else seq["gray"]
    dev = (hbm.put(frames), frames.strides[0], frames.strides[1]) if in_hbm else None
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        s = runner.Session(_lib.LIB_PATH, dict(seq, frames=seq["gray"]), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, threading=mode,
                           instance=instance or how == "replay" or group is not None, group=group, device_frames=dev, orientation=o)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    s._how = how
    return s, path


@pytest.fixture(scope="module")
def plain(seq):
    """mode -> (log, counters) of the plain run through the replay loop, taken before this module sets any orientation"""
    out = {}
    for mode in (0, 1):
        out[mode] = _finish(*_logged(seq, how="replay", mode=mode))
        F, B = _parse(out[mode][0])
        counts = out[mode][1]
        assert counts[0] == N == len(F)
        assert len(B) >= N - 70 and counts[3] >= 1 and counts[4] >= 10, counts   # tracking, marginalisations, keyframes
    return out


@pytest.mark.parametrize("in_hbm", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("mode", [0, 1], ids=["inline", "pipelined"])
def test_turned_frames_write_the_output_log_of_the_plain_run(seq, hbm, plain, mode, in_hbm):
    want = plain[mode]
    for o in (REVERSING, TRANSPOSING):
        got, c = _finish(*_logged(seq, o, "replay", in_hbm, mode, hbm=hbm))
        assert c == want[1], o
        assert got == want[0], "orientation %d: the output log differs from the plain run's (%d vs %d bytes)" % (o, len(got), len(want[0]))
    # and the plain run itself is what it was before any turned upload of this process
    again = _finish(*_logged(seq, how="replay", mode=mode))
    assert again == want, "the plain run changed after turned uploads"


def test_frame_by_frame_pushes_equal_the_replay_loop(seq, hbm, plain):
    """XRSLAMPushSensorData(XRSLAM_SENSOR_CAMERA) from the process-global instance and XRSLAMAmdPushImageDevice honour the setting"""
    got, c = _finish(*_logged(seq, TRANSPOSING, "step", False, 0))
    assert c == plain[0][1] and got == plain[0][0]
    got, c = _finish(*_logged(seq, REVERSING, "step", True, 0, hbm=hbm, instance=True))
    assert c == plain[0][1] and got == plain[0][0]
    # a new process-global instance starts upright again
    got, c = _finish(*_logged(seq, 0, "step", False, 0))
    assert c == plain[0][1] and got == plain[0][0]


def test_frame_by_frame_pushes_in_pipelined_mode_equal_the_replay_loop(seq, hbm, plain):
    """The orientation is bound to a frame when it is pushed: step-wise pushes with the backend running beside the next frame's tracker"""
    got, c = _finish(*_logged(seq, REVERSING, "step", False, 1))
    assert c == plain[1][1] and got == plain[1][0]
    got, c = _finish(*_logged(seq, TRANSPOSING, "step", True, 1, hbm=hbm, instance=True))
    assert c == plain[1][1] and got == plain[1][0]


def test_a_bad_orientation_mid_stream_is_reported_and_the_run_continues(seq):
    from xrslam_amd import _lib
    s = runner.Session(_lib.LIB_PATH, dict(seq, frames=seq["gray"]), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, orientation=TRANSPOSING)
    assert s.api.get_frame_orientation() == TRANSPOSING
    assert s.step() and s.step()
    assert not s.error(), s.error()
    for bad in (8, -1):
        assert s.api.set_frame_orientation(bad) == 0
        assert "orientation" in s.error() and str(bad) in s.error(), s.error()
        assert s.api.get_frame_orientation() == TRANSPOSING     # the setting stays
    assert s.step() and s.step()                                # the turned frames still fit: the library goes on
    # a frame that does not fit the orientation is dropped like any other bad frame: the 240-byte rows are too short for upright frames
    s.set_frame_orientation(0)
    assert s.step()
    assert "stride" in s.error(), s.error()
    s.set_frame_orientation(TRANSPOSING)
    assert s.step()
    s.flush()
    s.sync()
    assert s.times().frames == 5
    s.set_frame_orientation(0)                                   # (the process-global setting outlives the instance: leave it upright)
    s.close()


def test_turned_members_of_a_group_write_their_solo_logs(seq, hbm, plain):
    """Four members of one instance group: transposed host frames, mirrored frames in HBM, and two members that push plain frames (host,
    HBM).  Each writes its solo run's log -- which, for all four, is the plain run's."""
    from xrslam_amd import _lib
    plan = [(TRANSPOSING, False), (0, False), (MIRRORED, True), (0, True)]
    group = runner.Group(_lib.LIB_PATH)
    members = [_logged(seq, o, "step", in_hbm, group=group, hbm=hbm) for o, in_hbm in plan]
    res, errs = [None] * len(plan), []

    def work(i):
        try:
            res[i] = _finish(*members[i])
        except Exception as e:   # noqa: BLE001
            errs.append(repr(e))
    th = [threading.Thread(target=work, args=(i,)) for i in range(len(plan))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    group.close()
    assert not errs, errs
    for i, (got, c) in enumerate(res):
        assert c == plain[0][1], "member %d: counters" % i
        assert got == plain[0][0], "member %d (orientation %d): the grouped log differs from the solo plain log" % (i, plan[i][0])
