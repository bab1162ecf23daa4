"""Colour frames through the outer C API (include/XRSLAM.h) on the S1 stream.

The colour frames are built from the rendered gray frames by tests/color_frames.py: colorize (B = g, G = min(255, g + g//8),
R = g - g//4, alpha noise); G_ref = color_frames.gray_ref of them.  The device reduces a colour frame to exactly G_ref
(tests/test_color_gpu.py), so everything behind the gray plane is the same: the per-frame output log (tests/outlog.py) of a run
fed colour frames -- on any way into the library -- must be BYTE-identical to the log of the run fed G_ref as gray.  And against
the independent side: the CPU reference library (host arithmetic for the conversion, the oracle behind it) fed the same BGR frames,
under the comparison of tests/test_bench_stream_parity.py."""
import functools
import os
import tempfile
import threading

import numpy as np
import pytest

from tests import color_frames as cf
from tests import outlog
from tests.test_bench_stream_parity import BENCH_YAML, ORACLE_LIB, WORKERS, _assert_same_run, _run
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

N = 120   # initialises (60 seeded frames), fills the 10-keyframe window and marginalises (asserted below)


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    if not os.path.exists(ORACLE_LIB):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(os.path.dirname(ORACLE_LIB))])


@pytest.fixture(scope="module")
def seqs():
    """seed -> the rendered S1 stream, with its colour forms: 'bgr' (rows padded by 5 bytes), 'bgra' (dense), 'gray' = G_ref"""
    out = {}
    for seed in (1, 2):
        q = scene.make_sequence(n_frames=N, seed=seed, workers=WORKERS)
        bgr = cf.colorize(q["frames"], 3, pad=5)
        bgra = cf.colorize(q["frames"], 4)
        g = cf.gray_ref(bgr)
        np.testing.assert_array_equal(g, cf.gray_ref(bgra))
        assert len(np.unique(bgr[0].reshape(-1, 3), axis=0)) > 100 and (bgr[..., 1] != bgr[..., 2]).mean() > 0.9   # the channels differ
        out[seed] = dict(q, gray=g, bgr=bgr, bgra=bgra)
    return out


@pytest.fixture(scope="module")
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


def _logged(lib_path, seq, frames, channels, how="step", mode=0, undistort=None, group=None, instance=False, hbm=None):
    """One session over `frames`; how: 'step' (XRSLAM_SENSOR_CAMERA per frame), 'device' (frames in HBM, PushImageDevice[Color]),
    'replay' (XRSLAMAmdInstanceReplay[Color]).  -> (session, path of its output log)"""
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    dev = None
    if how == "device":
        dev = (hbm.put(frames), frames.strides[0], frames.strides[1])
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        s = runner.Session(lib_path, dict(seq, frames=frames), slam_yaml=BENCH_YAML, threading=mode, device_undistort=undistort,
                           channels=channels, instance=instance or how == "replay" or group is not None, group=group,
                           device_frames=dev)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    s._how = how
    return s, path


def _drain(s):
    if s._how == "replay":
        s.step_n(N)
        assert s.frame_k == N
    else:
        while s.step():
            assert not s.error(), s.error()
    s.flush()
    s.sync()
    assert not s.error(), s.error()
    t = s.times()
    counts = (t.frames, t.solves, t.solve_iterations, t.marginalizations, t.keyframes)
    s.close()
    return counts


def _finish(s, path):
    counts = _drain(s)
    with open(path, "rb") as fh:
        blob = fh.read()
    os.unlink(path)
    return blob, counts


@pytest.mark.parametrize("mode,undistort", [(0, None), (1, None), (0, "cv_undistort")], ids=["inline", "pipelined", "device_undistort"])
def test_colour_frames_write_the_output_log_of_their_gray_frames(seqs, hbm, mode, undistort):
    from xrslam_amd import _lib
    q = seqs[1]
    kw = dict(mode=mode, undistort=undistort, hbm=hbm)
    want, counts = _finish(*_logged(_lib.LIB_PATH, q, q["gray"], 1, **kw))
    F, B = _parse(want)
    assert counts[0] == N == len(F)
    if undistort is None:   # (rectifying frames the renderer did not distort bends the scene: identity is all that is asked there)
        assert len(B) >= N - 70 and counts[3] >= 1 and counts[4] >= 10, counts   # tracking, keyframes, marginalisations
    runs = {"bgr_host": (q["bgr"], 3, "step"), "bgra_host": (q["bgra"], 4, "step"), "bgra_hbm": (q["bgra"], 4, "device"),
            "bgr_replay": (q["bgr"], 3, "replay")}
    for name, (frames, channels, how) in runs.items():
        got, c = _finish(*_logged(_lib.LIB_PATH, q, frames, channels, how, **kw))
        assert c == counts, name
        assert got == want, "%s: the output log differs from the gray run's (%d vs %d bytes)" % (name, len(got), len(want))


def _parse(blob):
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    with os.fdopen(fd, "wb") as fh:
        fh.write(blob)
    try:
        return outlog.read(path)
    finally:
        os.unlink(path)


@pytest.mark.parametrize("channel", [2, 5])
def test_unsupported_channel_count_is_reported_and_the_frame_does_not_arrive(seqs, channel):
    from xrslam_amd import _lib
    q = seqs[1]
    s = runner.Session(_lib.LIB_PATH, dict(q, frames=q["bgra"]), slam_yaml=BENCH_YAML, channels=channel)
    assert s.step()
    assert "Image channel is not supported!" in s.error()
    assert s.times().frames == 0
    s.channels = 4                                         # the library goes on with the next (supported) frame
    assert s.step() and s.step()
    s.flush()
    s.sync()
    assert s.times().frames == 2
    s.close()


def test_gpu_matches_the_cpu_reference_on_bgr_frames(seqs, monkeypatch):
    """The GPU library's output for BGR host frames against the CPU reference library's for the same frames: ids equal, states and
    landmarks within 1e-4 (tests/test_bench_stream_parity.py: _assert_same_run)."""
    from xrslam_amd import _lib
    q = seqs[1]
    seq = dict(q, frames=q["bgr"])
    monkeypatch.setattr(runner, "Session", functools.partial(runner.Session, channels=3))
    marks = (76, 116)
    want = _run(ORACLE_LIB, seq, BENCH_YAML, 0, marks)
    assert want[1][0] == N and want[1][3] >= 1
    _assert_same_run(_run(_lib.LIB_PATH, seq, BENCH_YAML, 0, marks), want, seq, 0.03, "s1_bgr_inline")


def test_a_group_of_gray_bgr_and_bgra_members_shares_the_upload_launch(seqs, hbm):
    """Four members of one instance group -- gray host, BGR host, BGRA host, BGRA resident -- each write their solo run's log, and
    the launches that carry the frames' uploads (the preprocessing request, or an upload request of its own) served more than
    one member on average."""
    from xrslam_amd import _lib
    plan = [(seqs[1], "gray", 1, "step"), (seqs[2], "bgr", 3, "step"), (seqs[1], "bgra", 4, "step"), (seqs[2], "bgra", 4, "device")]
    solo = [_finish(*_logged(_lib.LIB_PATH, q, q[key], ch, how, instance=True, hbm=hbm)) for q, key, ch, how in plan]
    group = runner.Group(_lib.LIB_PATH)
    members = [_logged(_lib.LIB_PATH, q, q[key], ch, how, group=group, hbm=hbm) for q, key, ch, how in plan]
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
        assert got == want, "member %d (%s): the grouped log differs from the solo log" % (i, plan[i][1])
    assert solo[0][0] == solo[2][0] and solo[1][0] == solo[3][0]         # and colour members write their gray twin's log
    carried = [k for k in ("upload", "preprocess") if k in stats]
    assert carried, stats
    kind = "preprocess" if "preprocess" in stats else "upload"         # the upload rides with the preprocessing request
    assert stats[kind]["requests"] >= 4 * N and stats[kind]["requests"] / stats[kind]["batches"] > 1, stats
