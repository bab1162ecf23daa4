"""Masks through the outer C API (include/XRSLAM.h: XRSLAMAmdSetMask, XRSLAMAmdSetNextFrameMask) on the short 320x240 synthetic
stream (tests/golden/small_sensor_320.yaml), about 40 frames past the 60 seeded ones.

  * a static mask hiding the left third: no key point of any frame has its nearest pixel on a zero byte, the state reaches
    TRACKING_SUCCESS, and the key-point count is back at the configured budget at the end.  The budget is 30 (a 320x240 frame cannot
    hold 150 corners 20 pixels apart, let alone two thirds of it); that the visible two thirds hold enough texture for it is checked
    first, on the CPU, with tests/mask_model.py (uncapped) over the oracle's CLAHE image and Harris plane of frames of the stream;
  * an all-ones static mask writes the unmasked run's output log (tests/outlog.py), byte for byte, inline and pipelined;
  * a per-frame mask affects exactly its frame."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

from oracle import klt_oracle as ko
from tests import mask_model as mm
from tests import outlog
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR_YAML = os.path.join(ROOT, "tests", "golden", "small_sensor_320.yaml")
W, H = 320, 240
N = 100
BUDGET = 30
SEED = 1


@pytest.fixture(scope="module")
def seq():
    return scene.make_sequence(n_frames=N, seed=SEED, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))


@pytest.fixture(scope="module")
def slam_budget(tmp_path_factory):
    text = open(BENCH_YAML).read()
    key = "  max_keypoint_detection: 150\n"
    assert text.count(key) == 1
    path = tmp_path_factory.mktemp("mask") / "slam_budget.yaml"
    path.write_text(text.replace(key, "  max_keypoint_detection: %d\n" % BUDGET))
    return str(path)


def left_third():
    m = np.full((H, W), 255, np.uint8)
    m[:, :W // 3] = 0
    return m


def _session(seq, slam=BENCH_YAML, mode=0, log=False):
    from xrslam_amd import _lib
    path = None
    if log:
        fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
        os.close(fd)
        os.environ["XRSLAM_AMD_DUMP_OUT"] = path   # read when the session's pipeline is constructed
    try:
        s = runner.Session(_lib.LIB_PATH, seq, slam_yaml=slam, sensor_yaml=SENSOR_YAML, threading=mode)
    finally:
        os.environ.pop("XRSLAM_AMD_DUMP_OUT", None)
    return s, path


def _run(s, path, before_frame=None):
    """Plays the whole stream -> the output log's bytes; before_frame(k) runs ahead of frame k's push"""
    k = 0
    while True:
        if before_frame:
            before_frame(k)
        if not s.step():
            break
        assert not s.error(), s.error()
        k += 1
    s.flush()
    s.sync()
    assert not s.error(), s.error()
    frames = s.times().frames
    s.close()
    with open(path, "rb") as fh:
        blob = fh.read()
    os.unlink(path)
    assert frames == N
    return blob


def test_static_mask_keeps_every_key_point_off_the_hidden_third(seq, slam_budget):
    mask = left_third()
    for k in (60, 80, N - 1):   # condition, not measurement: the visible part holds the budget
        o = ko.OracleImage(seq["frames"][k])
        o.preprocess()
        # (max_points 0: every corner the visible part offers at 20 pixels' spacing -- 65 on these frames; a detection capped at the
        # budget returns fewer than the budget on its own, because the border rule is applied behind the cap)
        assert len(mm.detect(ko.harris_response(o.image), mask, np.zeros((0, 2)), 0, 20.0)) >= BUDGET, k
    s, _ = _session(seq, slam=slam_budget)
    assert s.set_mask(mask), s.error()
    counts, states = [], []
    while s.step():
        assert not s.error(), s.error()
        t, f = s.features()
        if t is None:
            continue
        xy = np.stack([f["x"], f["y"]], axis=1)
        assert not mm.on_zero_byte(xy, mask).any(), "frame %d" % s.frame_k
        counts.append(len(f))
        st = C.c_int(-1)
        s.api.get_result(runner.XRSLAM_RESULT_STATE, C.byref(st))
        states.append(st.value)
    s.close()
    assert len(counts) >= N - 2 and states[-1] == 1 and len(s.poses) >= 20, (len(counts), states[-5:])
    print("key points per frame, last ten:", counts[-10:])
    assert counts[-1] >= BUDGET, counts[-10:]


@pytest.mark.parametrize("mode", [0, 1], ids=["inline", "pipelined"])
def test_all_ones_static_mask_writes_the_unmasked_output_log(seq, mode):
    plain = _run(*_session(seq, mode=mode, log=True))
    s, path = _session(seq, mode=mode, log=True)
    assert s.set_mask(np.ones((H, W), np.uint8)), s.error()
    masked = _run(s, path)
    F, B = _parse(plain)
    assert len(F) == N and len(B) >= 20
    assert masked == plain, "%d vs %d bytes" % (len(masked), len(plain))


def _parse(blob):
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    with os.fdopen(fd, "wb") as fh:
        fh.write(blob)
    try:
        return outlog.read(path)
    finally:
        os.unlink(path)


def test_a_per_frame_mask_affects_exactly_its_frame(seq):
    K = 80
    mask = np.full((H, W), 1, np.uint8)
    mask[:, :W // 2] = 0
    plain, _ = _parse(_run(*_session(seq, log=True)))
    s, path = _session(seq, log=True)

    def before(k):
        if k == K:
            assert s.set_next_frame_mask(mask), s.error()

    got, _ = _parse(_run(s, path, before))
    assert len(got) == len(plain) == N
    for k in range(K):
        assert got[k]["px"].tobytes() == plain[k]["px"].tobytes() and got[k]["track"].tobytes() == plain[k]["track"].tobytes(), k
    assert mm.on_zero_byte(plain[K]["px"], mask).sum() > 5            # the unmasked run has key points there ...
    assert not mm.on_zero_byte(got[K]["px"], mask).any()              # ... the masked frame has none ...
    assert len(got[K]["px"]) > 5
    assert mm.on_zero_byte(got[K + 1]["px"], mask).sum() > 0          # ... and the next frame detects there again
