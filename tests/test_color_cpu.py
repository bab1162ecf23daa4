"""Colour frames on the CPU reference build, and the colour entry points' place in the ABI.

oracle/_build/libxrslam_oracle.so compiles the product's host sources against the xrhip shim, which has the gray uploads only:
the host sources reach the colour uploads through weak references and, where they are absent, reduce a colour frame themselves --
gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14.  That host arithmetic is the independent side the device conversion is compared
against (tests/test_color_stream_gpu.py); here it is pinned: BGR / BGRA frames (padded rows, alpha noise) give the output log of
their G_ref (tests/color_frames.py) pushed as gray, byte for byte, on every way into the library."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import color_frames as cf
from tests import outlog
from xrslam_amd.harness import runner, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "libxrslam_oracle.so")
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
N = 72


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    if not os.path.exists(ORACLE_LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


@pytest.fixture(scope="module")
def seq():
    q = scene.make_sequence(n_frames=N, seed=1)
    bgr, bgra = cf.colorize(q["frames"], 3, pad=5), cf.colorize(q["frames"], 4, pad=64)
    return dict(q, gray=cf.gray_ref(bgr), bgr=bgr, bgra=bgra)


def _run(seq, frames, channels, how="step"):
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        dev = (frames.ctypes.data, frames.strides[0], frames.strides[1]) if how == "device" else None   # "device" == host in the shim
        s = runner.Session(ORACLE_LIB, dict(seq, frames=frames), slam_yaml=BENCH_YAML, channels=channels, instance=how == "replay",
                           device_frames=dev)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    states = []
    if how == "replay":
        s.step_n(N)
    else:
        while s.step():
            assert not s.error(), s.error()
            st = C.c_int(-1)
            s.api.get_result(runner.XRSLAM_RESULT_STATE, C.byref(st))
            states.append(st.value)
    s.flush()
    s.sync()
    assert not s.error(), s.error()
    frames_done = s.times().frames
    s.close()
    with open(path, "rb") as fh:
        blob = fh.read()
    log = outlog.read(path)
    os.unlink(path)
    return blob, log, states, frames_done


def test_cpu_reference_reduces_colour_frames_to_their_gray_frame(seq):
    np.testing.assert_array_equal(seq["gray"], cf.gray_ref(seq["bgra"]))
    want, (F, B), states, done = _run(seq, seq["gray"], 1)
    assert done == N == len(F) and len(B) >= 5
    assert 1 in states, "G_ref does not carry the tracker to TRACKING_SUCCESS within %d frames" % N   # XRSLAM_STATE_TRACKING_SUCCESS
    assert min(len(f["px"]) for f in F[5:]) > 60                    # the mixes keep the texture
    for name, frames, channels, how in (("bgr", seq["bgr"], 3, "step"), ("bgra", seq["bgra"], 4, "step"),
                                        ("bgra through PushImageDeviceColor", seq["bgra"], 4, "device"),
                                        ("bgr through InstanceReplayColor", seq["bgr"], 3, "replay")):
        got = _run(seq, frames, channels, how)
        assert got[3] == N, name
        assert got[0] == want, "%s: the output log differs from the gray run's" % name


@pytest.mark.parametrize("channel", [2, 5])
def test_cpu_reference_reports_an_unsupported_channel_count(seq, channel):
    s = runner.Session(ORACLE_LIB, dict(seq, frames=seq["bgra"]), slam_yaml=BENCH_YAML, channels=channel)
    assert s.step()
    assert "Image channel is not supported!" in s.error()
    assert s.times().frames == 0
    s.close()


CALLER = r"""
#include "XRSLAM.h"
#include "xrslam_hip.h"
int call_color(xrhip_image *img, XRSLAMAmdInstance *inst, const void *px, const double *imu7, const double *cam_t, int *cur) {
    int rc = xrhip_image_upload_color(img, px, 752 * 3, 3, 0);
    rc += xrhip_image_upload_color_distorted(img, px, 752 * 4, 4, 1);
    XRSLAMAmdPushImageDeviceColor(px, 752 * 4, 4, 0.5);
    XRSLAMAmdInstancePushImageDeviceColor(inst, px, 752 * 3, 3, 0.5);
    return rc + XRSLAMAmdInstanceReplayColor(inst, imu7, 1, cam_t, 1, px, (size_t)752 * 480 * 3, 752 * 3, 3, 0, cur, cur + 1, 1, 0);
}
"""
NEW_SYMBOLS = ("xrhip_image_upload_color", "xrhip_image_upload_color_distorted", "XRSLAMAmdPushImageDeviceColor",
               "XRSLAMAmdInstancePushImageDeviceColor", "XRSLAMAmdInstanceReplayColor")


def test_colour_entry_points_are_declared_for_c_and_exported(tmp_path):
    """A C caller (not C++) compiles against include/XRSLAM.h and include/xrslam_hip.h, and the product library exports what it
    calls; the CPU reference build exports the outer three and leaves the two inner ones weak and undefined."""
    from xrslam_amd import _lib
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++17")):
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I" + os.path.join(ROOT, "include"), "-c",
                               str(src), "-o", str(tmp_path / ("caller_%s.o" % cc))])
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    ref = C.CDLL(ORACLE_LIB)                                # loads with immediate binding although the shim has no colour upload
    assert all(hasattr(ref, s) for s in NEW_SYMBOLS[2:]) and not any(hasattr(ref, s) for s in NEW_SYMBOLS[:2])
