"""Frames larger than cam0.resolution without a GPU: the CPU reference build.

oracle/_build/libxrslam_oracle.so compiles the product's host sources against the xrhip shim, which has no scaled upload: the host
sources reach xrhip_image_upload_scaled through weak references and, where it is absent, crop and area-average the frame
themselves with xrslam_amd/csrc/host/pixel_format.hpp: scale_frame.  Here that host arithmetic is pinned to tests/scale_model.py
through the outer API: a stream pushed scaled writes, byte for byte, the output log of the model's planes pushed as gray."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import color_frames as cf
from tests import pixfmt_model as pm
from tests import scale_model as sm
from xrslam_amd.harness import runner, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "libxrslam_oracle.so")
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR_YAML = os.path.join(ROOT, "tests", "golden", "small_sensor_320.yaml")
N = 72
W, H = 320, 240
GEO_2X2 = (2 * W, 2 * H, 0, 0, 2 * W, 2 * H)
GEO_3X2 = (3 * W + 7, 2 * H + 3, 5, 2, 3 * W, 2 * H)
GEO_ODD = (437, 331, 9, 4, 421, 323)


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


@pytest.fixture(scope="module")
def seq():
    q = scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))
    g = q["frames"]
    x3 = np.random.RandomState(5).randint(0, 256, size=(N, GEO_3X2[1], GEO_3X2[0]), dtype=np.uint8)
    x3[:, 2:2 + 2 * H, 5:5 + 3 * W] = sm.replicate(g, 3, 2)
    ys, xs = np.arange(GEO_ODD[1]) * H // GEO_ODD[1], np.arange(GEO_ODD[0]) * W // GEO_ODD[0]
    odd = cf.strided(pm.encode(np.ascontiguousarray(g[:, ys][:, :, xs]), pm.YUYV), 5)
    return dict(q, gray=g, x2=sm.replicate(g, 2, 2), x3=x3, odd=odd, odd_model=sm.scale(odd, GEO_ODD, W, H, pm.YUYV))


def _run(seq, frames, geometry=None, pixel_format=None, how="step"):
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        s = runner.Session(ORACLE_LIB, dict(seq, frames=frames), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, geometry=geometry,
                           pixel_format=pixel_format, instance=how == "replay")
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
    done = s.times().frames
    s.close()
    with open(path, "rb") as fh:
        blob = fh.read()
    os.unlink(path)
    return blob, states, done


def test_cpu_reference_scales_streams_to_the_models_planes(seq):
    want, states, done = _run(seq, seq["gray"])
    assert done == N and 1 in states, "the gray stream does not reach TRACKING_SUCCESS within %d frames" % N
    for name, key, geo, how in (("2x2", "x2", GEO_2X2, "step"), ("3x2 inside a larger frame, InstanceReplayScaled", "x3", GEO_3X2, "replay")):
        got = _run(seq, seq[key], geo, None, how)
        assert got[2] == N, name
        assert got[0] == want, "%s: the output log differs from the plain run's" % name
    want_odd = _run(seq, seq["odd_model"])
    got = _run(seq, seq["odd"], GEO_ODD, "yuyv")
    assert got[2] == N == want_odd[2]
    assert got[0] == want_odd[0], "yuyv, 421x323 -> 320x240: the output log differs from the run of the model's planes"
    assert want_odd[0] != want


@pytest.mark.parametrize("bad,word", [((2 * W, 2 * H, 1, 0, 2 * W, 2 * H), "crop"), ((2 * W, 2 * H, 0, 1, 2 * W, 2 * H), "crop"),
                                      ((2 * W, 2 * H, 0, 0, W - 1, 2 * H), "crop_width"), ((2 * W, 2 * H, 0, 0, 2 * W, H - 1), "crop_height"),
                                      ((5000, 5000, 0, 0, 4097, 4096), "2^24"), ((2 * W + 6, 2 * H, 0, 0, 2 * W, 2 * H), "stride")])
def test_cpu_reference_reports_a_bad_geometry_and_goes_on(seq, bad, word):
    s = runner.Session(ORACLE_LIB, dict(seq, frames=seq["x2"]), slam_yaml=BENCH_YAML, sensor_yaml=SENSOR_YAML, geometry=bad)
    assert s.step()
    assert "Image geometry is not supported" in s.error() and word in s.error(), s.error()
    assert s.times().frames == 0
    s.geometry = runner.frame_geometry(GEO_2X2)                # the library goes on with the next frame
    assert s.step() and s.step()
    s.flush()
    s.sync()
    assert s.times().frames == 2
    s.close()


CALLER = r"""
#include "XRSLAM.h"
#include "xrslam_hip.h"
int call_scaled(xrhip_image *img, XRSLAMAmdInstance *inst, const void *px, const double *imu7, const double *cam_t, int *cur) {
    XRSLAMAmdFrameFormat f = {XRSLAM_AMD_PIXEL_NV12, 0, 1};
    XRSLAMAmdFrameGeometry g = {1920, 1080, 114, 0, 1692, 1080};
    xrhip_frame_geometry gi = {1920, 1080, 114, 0, 1692, 1080};
    double k[4] = {1400, 1400, 960, 540}, o[4];
    int rc = xrhip_image_upload_scaled(img, px, 1920, XRHIP_PIXFMT_NV12, 0, 1, 0, &gi);
    rc += xrhip_image_upload_scaled_distorted(img, px, 1920, XRHIP_PIXFMT_NV12, 0, 0, 1, &gi);
    XRSLAMAmdPushImageScaled(px, 1920, &f, &g, 1, 0.5);
    XRSLAMAmdPushImageScaled(px, 1920, 0, &g, 0, 0.5);
    XRSLAMAmdInstancePushImageScaled(inst, px, 1920, &f, &g, 0, 0.5);
    XRSLAMAmdScaleIntrinsics(k, &g, 752, 480, o);
    return rc + XRSLAMAmdInstanceReplayScaled(inst, imu7, 1, cam_t, 1, px, (size_t)1920 * 1620, 1920, &f, &g, 0, cur, cur + 1, 1, 0);
}
int same_layout[sizeof(XRSLAMAmdFrameGeometry) == sizeof(xrhip_frame_geometry) ? 1 : -1];
"""
NEW_SYMBOLS = ("xrhip_image_upload_scaled", "xrhip_image_upload_scaled_distorted", "XRSLAMAmdPushImageScaled",
               "XRSLAMAmdInstancePushImageScaled", "XRSLAMAmdInstanceReplayScaled", "XRSLAMAmdScaleIntrinsics")


def test_scaled_entry_points_are_declared_for_c_and_exported(tmp_path):
    """A C caller compiles against include/XRSLAM.h and include/xrslam_hip.h; the product library exports what it calls; the CPU
    reference build exports the outer four and leaves the two inner ones weak and undefined."""
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
    ref = C.CDLL(ORACLE_LIB)
    assert all(hasattr(ref, s) for s in NEW_SYMBOLS[2:]) and not any(hasattr(ref, s) for s in NEW_SYMBOLS[:2])
