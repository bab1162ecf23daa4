"""Bayer mosaics through the outer C API (include/XRSLAM.h: XRSLAMAmdPushImageFormat) on the short 320x240 synthetic stream of
tests/test_pixfmt_stream_gpu.py.

The device demosaics a mosaic to exactly the model's gray plane (tests/test_bayer_gpu.py against tests/bayer_model.py), so everything
behind the gray plane is the same: the output log (tests/outlog.py) of a run pushed BAYER_GRBG8 mosaics must be BYTE-identical to the
log of the run pushed the model's gray planes through the plain camera push -- alone and as a member of a two-instance group."""
import threading

import pytest

from tests import bayer_model as bm
from tests import color_frames as cf
from tests.test_color_stream_gpu import N, _finish, _parse
from tests.test_pixfmt_stream_gpu import H, W, _logged
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seq():
    """The rendered stream as the GRBG mosaic of its colourised frames (rows padded by 5 bytes), and the model's gray planes of it"""
    q = scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))
    mosaic = cf.strided(bm.encode(q["frames"], bm.GRBG8), 5)
    g = bm.reduce(mosaic, bm.GRBG8)
    assert (g != q["frames"]).mean() > 0.5 and (mosaic[..., 0] != g).mean() > 0.5      # neither the scene's gray nor the raw samples
    return dict(q, gray=g, bayer=mosaic)


@pytest.fixture(scope="module")
def hbm():
    h = cf.Hbm()
    yield h
    h.close()


def test_bayer_stream_writes_the_output_log_of_the_models_gray_planes(seq, hbm):
    want, counts = _finish(*_logged(seq, "gray"))
    F, B = _parse(want)
    assert counts[0] == N == len(F)
    assert len(B) >= N - 70 and counts[3] >= 1 and counts[4] >= 10, counts   # tracking, marginalisations, keyframes
    for name, in_hbm in (("host", False), ("HBM", True)):
        got, c = _finish(*_logged(seq, "bayer", "bayer_grbg8", "step", in_hbm, hbm=hbm))
        assert c == counts, name
        assert got == want, "%s: the output log differs from the gray run's (%d vs %d bytes)" % (name, len(got), len(want))


def test_a_bayer_member_of_a_group_writes_its_solo_log(seq, hbm):
    """Two members of one instance group -- the gray planes through the plain push, the mosaics through the format push -- write
    the same log, the one each writes alone: the Bayer launch goes out in the member's order, behind its shared upload."""
    from xrslam_amd import _lib
    plan = [("gray", None), ("bayer", "bayer_grbg8")]
    solo = [_finish(*_logged(seq, key, fmt, "step", instance=True)) for key, fmt in plan]
    group = runner.Group(_lib.LIB_PATH)
    members = [_logged(seq, key, fmt, "step", group=group) for key, fmt in plan]
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
