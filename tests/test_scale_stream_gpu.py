"""Frames larger than cam0.resolution through the outer C API (include/XRSLAM.h: XRSLAMAmdPushImageScaled,
XRSLAMAmdInstanceReplayScaled) on the short 320x240 synthetic stream of tests/test_pixfmt_stream_gpu.py.

A frame whose pixels are replicated k x k scales back to the original bits (tests/test_scale_model.py), so everything behind the
gray plane is the same: a run pushed 2x2-replicated (640x480) or 3x2-replicated (960x480) frames must write the BYTE-identical
output log (tests/outlog.py) of the plain gray run -- inline and pipelined, from host memory and from HBM, alone and as one member of
an instance group whose other members push plain frames.  A non-integer geometry is held to the run that is pushed the model's
planes (tests/scale_model.py) as GRAY8."""
import os
import tempfile
import threading

import numpy as np
import pytest

from tests import color_frames as cf
from tests import scale_model as sm
from tests.test_color_stream_gpu import N, _finish, _parse   # N: leaves initialisation, fills the window, marginalises (asserted below)
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR_YAML = os.path.join(ROOT, "tests", "golden", "small_sensor_320.yaml")
W, H = 320, 240
GEO_2X2 = (2 * W, 2 * H, 0, 0, 2 * W, 2 * H)
GEO_3X2 = (3 * W + 7, 2 * H + 3, 5, 2, 3 * W, 2 * H)          # the replicated frame sits inside a larger one
GEO_ODD = (437, 331, 9, 4, 421, 323)                           # 421 -> 320, 323 -> 240: coprime, non-integer


@pytest.fixture(scope="module")
def seq():
    q = scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))
    g = q["frames"]
    x3 = np.random.RandomState(5).randint(0, 256, size=(N, GEO_3X2[1], GEO_3X2[0]), dtype=np.uint8)
    x3[:, 2:2 + 2 * H, 5:5 + 3 * W] = sm.replicate(g, 3, 2)
    # a larger rendering of the same scene would do; bytes that follow the scene are enough: the small frame, enlarged by
    # repetition of rows and columns to 437 x 331 (what the model makes of it is the reference, whatever it shows)
    ys, xs = np.arange(GEO_ODD[1]) * H // GEO_ODD[1], np.arange(GEO_ODD[0]) * W // GEO_ODD[0]
    odd = np.ascontiguousarray(g[:, ys][:, :, xs])
    out = dict(q, gray=g, x2=cf.strided(sm.replicate(g, 2, 2)[..., None], 5)[..., 0], x3=x3, odd=odd, odd_model=sm.scale_gray(odd, GEO_ODD, W, H))
    np.testing.assert_array_equal(sm.scale_gray(out["x2"], GEO_2X2, W, H), g)
    np.testing.assert_array_equal(sm.scale_gray(x3, GEO_3X2, W, H), g)
    assert (out["odd_model"] != g).mean() > 0.2
    return out


@pytest.fixture(scope="module")
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


def _logged(seq, key, geometry=None, how="step", in_hbm=False, mode=0, group=None, instance=False, hbm=None, pixel_format=None):
    from xrslam_amd import _lib
    frames = seq[key]
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    dev = (hbm.put(frames), frames.strides[0], frames.strides[1]) if in_hbm else None
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        s = runner.Session(_lib.LIB_PATH, dict(seq, frames=frames), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, threading=mode,
                           geometry=geometry, pixel_format=pixel_format, instance=instance or how == "replay" or group is not None,
                           group=group, device_frames=dev)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    s._how = how
    return s, path


@pytest.fixture(scope="module")
def plain(seq):
    """mode -> (log, counters) of the plain gray run through the replay loop, taken before this module makes any scaled call"""
    out = {}
    for mode in (0, 1):
        out[mode] = _finish(*_logged(seq, "gray", how="replay", mode=mode))
        F, B = _parse(out[mode][0])
        counts = out[mode][1]
        assert counts[0] == N == len(F)
        assert len(B) >= N - 70 and counts[3] >= 1 and counts[4] >= 10, counts   # tracking, marginalisations, keyframes
    return out


@pytest.mark.parametrize("in_hbm", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("mode", [0, 1], ids=["inline", "pipelined"])
def test_replicated_frames_write_the_output_log_of_the_plain_run(seq, hbm, plain, mode, in_hbm):
    want = plain[mode]
    for name, key, geo in (("2x2", "x2", GEO_2X2), ("3x2", "x3", GEO_3X2)):
        got, c = _finish(*_logged(seq, key, geo, "replay", in_hbm, mode, hbm=hbm))
        assert c == want[1], name
        assert got == want[0], "%s: the output log differs from the plain run's (%d vs %d bytes)" % (name, len(got), len(want[0]))
    # and the plain run itself is what it was before any scaled call of this process
    again = _finish(*_logged(seq, "gray", how="replay", mode=mode))
    assert again == want, "the plain run changed after scaled uploads"


def test_frame_by_frame_pushes_equal_the_replay_loop(seq, hbm, plain):
    got, c = _finish(*_logged(seq, "x2", GEO_2X2, "step", True, 0, hbm=hbm))
    assert c == plain[0][1] and got == plain[0][0]
    got, c = _finish(*_logged(seq, "x3", GEO_3X2, "step", False, 0, instance=True))
    assert c == plain[0][1] and got == plain[0][0]


@pytest.mark.parametrize("in_hbm", [False, True], ids=["host", "hbm"])
def test_a_non_integer_geometry_equals_the_run_of_the_models_planes(seq, hbm, in_hbm):
    want = _finish(*_logged(seq, "odd_model", how="replay", pixel_format="gray8"))
    F, _ = _parse(want[0])
    assert want[1][0] == N == len(F)
    got = _finish(*_logged(seq, "odd", GEO_ODD, "replay", in_hbm, hbm=hbm))
    assert got[1] == want[1]
    assert got[0] == want[0], "the output log differs from the run pushed the model's planes"


@pytest.mark.parametrize("bad,word", [((2 * W, 2 * H, 1, 0, 2 * W, 2 * H), "crop"), ((2 * W, 2 * H, 0, 0, W - 1, 2 * H), "crop_width"),
                                      ((2 * W, 2 * H, 0, 0, 2 * W, H - 1), "crop_height"), ((2 * W + 6, 2 * H, 0, 0, 2 * W, 2 * H), "stride")])
def test_a_bad_geometry_mid_stream_is_reported_and_the_run_continues(seq, bad, word):
    from xrslam_amd import _lib
    s = runner.Session(_lib.LIB_PATH, dict(seq, frames=seq["x2"]), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, geometry=GEO_2X2)
    assert s.step() and s.step()
    assert not s.error(), s.error()
    good = s.geometry
    s.geometry = runner.frame_geometry(bad)
    assert s.step()
    assert "geometry" in s.error() and word in s.error(), s.error()
    s.geometry = good                                           # the library goes on with the next frame
    assert s.step() and s.step()
    s.flush()
    s.sync()
    assert s.times().frames == 4
    s.close()


def test_a_scaled_member_of_a_group_writes_its_solo_log(seq, hbm, plain):
    """Four members of one instance group: 2x2-replicated host frames, 3x2-replicated frames in HBM, and two members that push plain
    frames (host, HBM).  Each writes its solo run's log -- which, for all four, is the plain run's."""
    from xrslam_amd import _lib
    plan = [("x2", GEO_2X2, False), ("gray", None, False), ("x3", GEO_3X2, True), ("gray", None, True)]
    group = runner.Group(_lib.LIB_PATH)
    members = [_logged(seq, key, geo, "step", in_hbm, group=group, hbm=hbm) for key, geo, in_hbm in plan]
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
        assert got == plain[0][0], "member %d (%s): the grouped log differs from the solo plain log" % (i, plan[i][0])
