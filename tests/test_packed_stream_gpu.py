"""Packed 10 / 12-bit frames through the outer C API (include/XRSLAM.h: XRSLAMAmdPushImageFormat, XRSLAMAmdPushImageScaled) on a
short 320x240 synthetic stream (tests/golden/small_sensor_320.yaml).

A packed frame is defined as the frame of the same samples written as 16-bit values (tests/test_packed_gpu.py holds the device to
that, plane by plane), so the whole output log (tests/outlog.py) of a run pushed GRAY10_MIPI, GRAY12P or BAYER_RGGB10P frames must be
BYTE-identical to the log of the run pushed those samples as GRAY16 / BAYER_RGGB16 with bits 10 / 12 -- inline and pipelined, scaled,
and as a member of a two-member instance group."""
import os
import tempfile
import threading

import numpy as np
import pytest

from tests import bayer_model as bm
from tests import color_frames as cf
from tests import packed_model as pk
from tests import pixfmt_model as pm
from tests import scale_model as sm
from tests.test_color_stream_gpu import _finish, _parse
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR_YAML = os.path.join(ROOT, "tests", "golden", "small_sensor_320.yaml")
W, H = 320, 240
N = 40
GEO = (2 * W + 3, 2 * H + 2, 3, 1, 2 * W, 2 * H)     # the 2x frames sit at (3, 1) of a larger one: the crop starts mid-group
# name -> (the packed format, its 16-bit twin as frame_format takes it)
PLAN = {"gray10_mipi": ("gray16", 10), "gray12p": ("gray16", 12), "bayer_rggb10p": ("bayer_rggb16", 10)}


def _rows(samples, packing, pad):
    """[n][h][w] samples -> [n][h][row bytes] packed rows, `pad` bytes of 0xEE after each"""
    rows = np.stack([pk.pack(s, packing) for s in samples])
    buf = np.full(rows.shape[:2] + (rows.shape[2] + pad,), 0xEE, np.uint8)
    out = buf[:, :, :rows.shape[2]]
    out[...] = rows
    return out


@pytest.fixture(scope="module")
def seq():
    """The rendered stream as 10 / 12-bit samples (the gray value in the top 8 bits, seeded noise below; the mosaic: the colourised
    frame behind an RGGB filter), each as 16-bit frames and packed; and 2x frames inside a larger one for the scaled push."""
    q = scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))
    g = q["frames"]
    rs = np.random.RandomState(4)
    out = dict(q)
    for name, (twin, bits) in PLAN.items():
        fmt = runner.PACKED_PIXEL_FORMATS[name]
        if fmt in pk.MONO:
            s = (g.astype(np.int64) << (bits - 8)) | rs.randint(0, 1 << (bits - 8), size=g.shape)
        else:
            px16 = bm.encode(g, bm.RGGB16, bits)
            s = px16[..., 0].astype(np.int64) | (px16[..., 1].astype(np.int64) << 8)
        out[name + "/16"] = cf.strided(pm.samples16(s), 5)
        out[name] = _rows(s, pk.PACKING[fmt], 5)
        np.testing.assert_array_equal(pk.unpack(out[name][0], W, pk.PACKING[fmt]), s[0])
        big = np.zeros((N, GEO[1], GEO[0]), np.int64)
        big[...] = rs.randint(0, 1 << bits, size=big.shape)
        big[:, GEO[3]:GEO[3] + 2 * H, GEO[2]:GEO[2] + 2 * W] = sm.replicate(s, 2, 2)
        out[name + "/big16"] = pm.samples16(big)
        out[name + "/big"] = _rows(big, pk.PACKING[fmt], 0)
    return out


@pytest.fixture(scope="module")
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


def _logged(seq, key, pixel_format, mode=0, geometry=None, in_hbm=False, hbm=None, group=None, instance=False):
    from xrslam_amd import _lib
    frames = seq[key]
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    dev = (hbm.put(frames), frames.strides[0], frames.strides[1]) if in_hbm else None
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        s = runner.Session(_lib.LIB_PATH, dict(seq, frames=frames), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, threading=mode,
                           pixel_format=pixel_format, geometry=geometry, instance=instance or group is not None, group=group,
                           device_frames=dev)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    s._how = "step"
    return s, path


@pytest.mark.parametrize("mode", [0, 1], ids=["inline", "pipelined"])
@pytest.mark.parametrize("name", sorted(PLAN))
def test_packed_streams_write_the_output_log_of_their_16_bit_twins(seq, hbm, name, mode):
    want, counts = _finish(*_logged(seq, name + "/16", PLAN[name], mode))
    F, _ = _parse(want)
    assert counts[0] == N == len(F) and min(len(f["px"]) for f in F[5:]) > 20      # every frame arrived and was tracked
    for where, in_hbm in (("host", False), ("HBM", True)):
        got, c = _finish(*_logged(seq, name, name, mode, in_hbm=in_hbm, hbm=hbm))
        assert c == counts, where
        assert got == want, "%s, %s: the output log differs from the 16-bit run's (%d vs %d bytes)" % (name, where, len(got), len(want))


@pytest.mark.parametrize("mode", [0, 1], ids=["inline", "pipelined"])
@pytest.mark.parametrize("name", sorted(PLAN))
def test_scaled_packed_streams_write_the_output_log_of_their_16_bit_twins(seq, name, mode):
    want, counts = _finish(*_logged(seq, name + "/big16", PLAN[name], mode, GEO))
    F, _ = _parse(want)
    assert counts[0] == N == len(F) and min(len(f["px"]) for f in F[5:]) > 20
    got, c = _finish(*_logged(seq, name + "/big", name, mode, GEO))
    assert c == counts
    assert got == want, "%s: the output log differs from the 16-bit run's (%d vs %d bytes)" % (name, len(got), len(want))


def test_a_packed_member_of_a_group_writes_its_solo_log(seq):
    """Two members of one instance group -- 16-bit frames through the shared upload launch, the same samples packed through a launch
    of the member's own behind it -- write the same log, the one each writes alone."""
    from xrslam_amd import _lib
    plan = [("gray10_mipi/16", ("gray16", 10)), ("gray10_mipi", "gray10_mipi")]
    solo = [_finish(*_logged(seq, key, fmt, instance=True)) for key, fmt in plan]
    group = runner.Group(_lib.LIB_PATH)
    members = [_logged(seq, key, fmt, group=group) for key, fmt in plan]
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
    for i, ((want, cw), (got, cg)) in enumerate(zip(solo, res)):
        assert cw == cg and cw[0] == N, "member %d: counters" % i
        assert got == want, "member %d (%s): the grouped log differs from the solo log" % (i, plan[i][0])
    assert solo[0][0] == solo[1][0]


def test_a_bad_packed_frame_is_dropped_with_the_error_set(seq):
    from xrslam_amd import _lib
    short = np.ascontiguousarray(seq["gray12p"][:, :, :-1])      # rows one byte short of the packed row
    s = runner.Session(_lib.LIB_PATH, dict(seq, frames=short), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, pixel_format="gray12p")
    assert s.step()
    assert "stride" in s.error() and s.times().frames == 0
    s.pixel_format = runner.frame_format(("bayer_rggb10p", 0, 1))
    assert s.step()
    assert "limited_range" in s.error() and s.times().frames == 0
    s.close()
