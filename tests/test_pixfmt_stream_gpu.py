"""Camera pixel formats through the outer C API (include/XRSLAM.h: XRSLAMAmdPushImageFormat, XRSLAMAmdInstanceReplayFormat) on a
short 320x240 synthetic stream (tests/golden/small_sensor_320.yaml).

The device reduces a frame of any format to exactly the model's gray frame (tests/test_pixfmt_gpu.py against tests/pixfmt_model.py),
so everything behind the gray plane is the same: the output log (tests/outlog.py) of a run pushed GRAY16, YUYV, RGBA8 or
NV12 + limited_range frames must be BYTE-identical to the log of the run pushed the model's gray frames as gray -- inline and
pipelined, frame by frame and through the replay loop, alone and as a member of an instance group."""
import os
import tempfile
import threading

import numpy as np
import pytest

from tests import color_frames as cf
from tests import pixfmt_model as pm
from tests.test_color_stream_gpu import N, _finish, _parse   # N: leaves initialisation, fills the window, marginalises (asserted below)
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR_YAML = os.path.join(ROOT, "tests", "golden", "small_sensor_320.yaml")
W, H = 320, 240


@pytest.fixture(scope="module")
def seq():
    """The rendered stream and its forms.  'gray' = the model's reduction of the RGBA frames; GRAY16 (12 bits, rows padded by 5
    bytes: odd row addresses) and YUYV encode that gray frame; NV12 is a whole surface (luma rows, then chroma rows of noise) at
    video levels, whose gray twin is 'gray_nv12'."""
    q = scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))
    rgba = pm.encode(q["frames"], pm.RGBA8)
    g = pm.reduce(rgba, pm.RGBA8)
    nv12 = pm.encode(g, pm.NV12, 0, 1)
    surface = np.random.RandomState(8).randint(0, 256, size=(N, H + H // 2, W, 1), dtype=np.uint8)
    surface[:, :H] = nv12
    out = dict(q, gray=g, rgba8=rgba, gray16=cf.strided(pm.encode(g, pm.GRAY16, 12), 5), yuyv=cf.strided(pm.encode(g, pm.YUYV), 64),
               nv12=surface, gray_nv12=pm.reduce(nv12, pm.NV12, 0, 1))
    np.testing.assert_array_equal(pm.reduce(out["gray16"], pm.GRAY16, 12), g)
    np.testing.assert_array_equal(pm.reduce(out["yuyv"], pm.YUYV), g)
    assert (out["gray_nv12"] != g).any()
    return out


# name -> (frames, pixel_format, frames live in HBM, the gray twin)
PLAN = {"gray16_host": ("gray16", ("gray16", 12), False, "gray"), "yuyv_hbm": ("yuyv", "yuyv", True, "gray"),
        "rgba8_host": ("rgba8", "rgba8", False, "gray"), "nv12_limited_hbm": ("nv12", ("nv12", 0, 1), True, "gray_nv12")}


@pytest.fixture(scope="module")
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


def _logged(seq, key, pixel_format=None, how="step", in_hbm=False, mode=0, group=None, instance=False, hbm=None):
    from xrslam_amd import _lib
    frames = seq[key]
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    dev = (hbm.put(frames), frames.strides[0], frames.strides[1]) if in_hbm else None
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        s = runner.Session(_lib.LIB_PATH, dict(seq, frames=frames), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, threading=mode,
                           pixel_format=pixel_format, instance=instance or how == "replay" or group is not None, group=group,
                           device_frames=dev)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    s._how = how
    return s, path


@pytest.mark.parametrize("how", ["step", "replay"])
@pytest.mark.parametrize("mode", [0, 1], ids=["inline", "pipelined"])
def test_format_streams_write_the_output_log_of_their_gray_frames(seq, hbm, mode, how):
    want = {}
    for twin in ("gray", "gray_nv12"):
        want[twin] = _finish(*_logged(seq, twin, how=how, mode=mode))
        F, B = _parse(want[twin][0])
        counts = want[twin][1]
        assert counts[0] == N == len(F)
        assert len(B) >= N - 70 and counts[3] >= 1 and counts[4] >= 10, counts   # tracking, marginalisations, keyframes
    for name, (key, fmt, in_hbm, twin) in PLAN.items():
        got, c = _finish(*_logged(seq, key, fmt, how, in_hbm, mode, hbm=hbm))
        assert c == want[twin][1], name
        assert got == want[twin][0], "%s: the output log differs from the gray run's (%d vs %d bytes)" % (name, len(got), len(want[twin][0]))


@pytest.mark.parametrize("bad,word", [((99,), "format"), (("gray16", 17), "bits"), (("rgba8", 0, 1), "limited_range")])
def test_a_bad_format_is_reported_and_the_frame_does_not_arrive(seq, bad, word):
    from xrslam_amd import _lib
    s = runner.Session(_lib.LIB_PATH, dict(seq, frames=seq["rgba8"]), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, pixel_format=bad)
    assert s.step()
    assert word in s.error()
    assert s.times().frames == 0
    s.pixel_format = runner.frame_format("rgba8")          # the library goes on with the next (supported) frame
    assert s.step() and s.step()
    s.flush()
    s.sync()
    assert s.times().frames == 2
    s.close()


def test_a_group_of_four_formats_shares_the_upload_launch(seq, hbm):
    """Four members of one instance group -- plain gray host, GRAY16 host, YUYV resident, NV12 + limited_range resident -- each
    write their solo run's log, and the launches that carry the frames' uploads served more than one member on average."""
    plan = [("gray", None, False), ("gray16", ("gray16", 12), False), ("yuyv", "yuyv", True), ("nv12", ("nv12", 0, 1), True)]
    solo = [_finish(*_logged(seq, key, fmt, "step", in_hbm, instance=True, hbm=hbm)) for key, fmt, in_hbm in plan]
    from xrslam_amd import _lib
    group = runner.Group(_lib.LIB_PATH)
    members = [_logged(seq, key, fmt, "step", in_hbm, group=group, hbm=hbm) for key, fmt, in_hbm in plan]
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
    stats = group.stats()
    group.close()
    assert not errs, errs
    for i, ((want, cw), (got, cg)) in enumerate(zip(solo, res)):
        assert cw == cg and cw[0] == N, "member %d: counters" % i
        assert got == want, "member %d (%s): the grouped log differs from the solo log" % (i, plan[i][0])
    assert solo[0][0] == solo[1][0] == solo[2][0] and solo[3][0] != solo[0][0]   # and format members write their gray twin's log
    carried = [k for k in ("upload", "preprocess") if k in stats]
    assert carried, stats
    kind = "preprocess" if "preprocess" in stats else "upload"         # the upload rides with the preprocessing request
    assert stats[kind]["requests"] >= 4 * N and stats[kind]["requests"] / stats[kind]["batches"] > 1, stats
