"""Camera pixel formats without a GPU: the numpy model against hand-computed values, the CPU reference build, the ABI.

oracle/_build/libxrslam_oracle.so compiles the product's host sources against the xrhip shim, which has no format upload: the host
sources reach xrhip_image_upload_format through weak references and, where it is absent, reduce the frame themselves with the
formulas of xrslam_amd/csrc/host/pixel_format.hpp.  Here that host arithmetic is pinned to tests/pixfmt_model.py: a stream pushed in
a format writes the output log of the model's gray frames pushed as gray, byte for byte."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import color_frames as cf
from tests import outlog
from tests import pixfmt_model as pm
from xrslam_amd.harness import runner, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "libxrslam_oracle.so")
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
N = 72


# ------------------------------------------------------------------------------------------------ the model
def test_model_limited_range_by_hand():
    #   ((max(g,16) - 16) * 255 + 109) // 219:  17 -> 364 // 219;  126 -> 28159 // 219;  234 -> 55699 // 219;  236 -> 56209 // 219 = 256 -> 255
    got = pm.expand_limited(np.array([0, 15, 16, 17, 126, 234, 235, 236, 255]))
    np.testing.assert_array_equal(got, [0, 0, 0, 1, 128, 254, 255, 255, 255])
    px = np.array([0, 15, 16, 17, 126, 234, 235, 236, 255], np.uint8).reshape(1, 9, 1)
    for fmt in (pm.GRAY8, pm.NV12, pm.I420):
        np.testing.assert_array_equal(pm.reduce(px, fmt, 0, 1)[0], [0, 0, 0, 1, 128, 254, 255, 255, 255])
        np.testing.assert_array_equal(pm.reduce(px, fmt)[0], px[0, :, 0])


@pytest.mark.parametrize("bits,want", [(8, [0, 255, 255, 255]), (10, [0, 255, 255, 255]), (12, [0, 255, 255, 255]), (16, [0, 255, 255])])
def test_model_gray16_by_hand(bits, want):
    """Samples 0, 2^bits - 1, 2^bits, 65535 (2^16 is no sample): everything from 2^bits - 1 up saturates at 255."""
    v = [0, (1 << bits) - 1] + ([1 << bits] if bits < 16 else []) + [65535]
    px = pm.samples16(np.array(v)).reshape(1, len(v), 2)
    np.testing.assert_array_equal(pm.reduce(px, pm.GRAY16, bits)[0], want)
    if bits == 16:
        np.testing.assert_array_equal(pm.reduce(px, pm.GRAY16, 0)[0], want)       # 0 means 16
    # below saturation: the top eight of the significant bits
    mid = pm.samples16(np.array([0x1234 >> (16 - bits)])).reshape(1, 1, 2)
    assert pm.reduce(mid, pm.GRAY16, bits)[0, 0] == 0x12
    # little endian; P010 is the high byte, YUYV / UYVY pick byte 0 / 1
    two = np.array([0x34, 0x12], np.uint8).reshape(1, 1, 2)
    assert pm.reduce(two, pm.GRAY16, 16)[0, 0] == 0x12 and pm.reduce(two, pm.P010)[0, 0] == 0x12
    assert pm.reduce(two, pm.YUYV)[0, 0] == 0x34 and pm.reduce(two, pm.UYVY)[0, 0] == 0x12


def test_model_rgb_is_bgr_with_swapped_input():
    for c, (rgb, bgr) in ((3, (pm.RGB8, pm.BGR8)), (4, (pm.RGBA8, pm.BGRA8))):
        px = cf.random_pixels(31, 17, c, seed=c)
        swapped = np.ascontiguousarray(px[..., [2, 1, 0] + ([3] if c == 4 else [])])
        np.testing.assert_array_equal(pm.reduce(px, rgb), pm.reduce(swapped, bgr))
        np.testing.assert_array_equal(pm.reduce(swapped, bgr), cf.gray_ref(swapped))
        assert (pm.reduce(px, rgb) != pm.reduce(px, bgr)).mean() > 0.5
    one = np.array([[[255, 0, 0]]], np.uint8)                                   # pure R: (255 * 4899 + 8192) >> 14 = 76
    assert pm.reduce(one, pm.RGB8)[0, 0] == 76 and pm.reduce(one, pm.BGR8)[0, 0] == 29


# ------------------------------------------------------------------------------------------------ the CPU reference pipeline
@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


@pytest.fixture(scope="module")
def seq():
    q = scene.make_sequence(n_frames=N, seed=1)
    rgb = cf.strided(pm.encode(q["frames"], pm.RGB8), 5)
    g = pm.reduce(rgb, pm.RGB8)                                                  # the colour mix's gray: every other stream encodes it
    nv12 = pm.encode(g, pm.NV12, 0, 1)
    h = g.shape[1]
    surface = np.random.RandomState(8).randint(0, 256, size=(len(g), h + h // 2, g.shape[2], 1), dtype=np.uint8)   # luma + chroma rows
    surface[:, :h] = nv12
    return dict(q, gray=g, rgb8=rgb, gray16=cf.strided(pm.encode(g, pm.GRAY16, 10), 64), yuyv=cf.strided(pm.encode(g, pm.YUYV), 5),
                nv12=surface, gray_nv12=pm.reduce(nv12, pm.NV12, 0, 1))


def _run(seq, frames, pixel_format=None, how="step"):
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path              # read when the session's pipeline is constructed
    try:
        dev = (frames.ctypes.data, frames.strides[0], frames.strides[1]) if how == "device" else None   # "device" == host in the shim
        s = runner.Session(ORACLE_LIB, dict(seq, frames=frames), slam_yaml=BENCH_YAML, pixel_format=pixel_format, instance=how == "replay",
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


def test_cpu_reference_reduces_format_streams_to_the_models_gray_frames(seq):
    np.testing.assert_array_equal(seq["gray"], pm.reduce(seq["gray16"], pm.GRAY16, 10))
    np.testing.assert_array_equal(seq["gray"], pm.reduce(seq["yuyv"], pm.YUYV))
    assert (seq["gray_nv12"] != seq["gray"]).any()          # (video levels do not round-trip: that stream has a gray twin of its own)
    want, (F, B), states, done = _run(seq, seq["gray"])
    assert done == N == len(F) and len(B) >= 5
    assert 1 in states, "the gray stream does not reach TRACKING_SUCCESS within %d frames" % N
    assert min(len(f["px"]) for f in F[5:]) > 60
    for name, frames, fmt, how in (("gray16, 10 bits", seq["gray16"], ("gray16", 10), "step"), ("yuyv, on_device", seq["yuyv"], "yuyv", "device"),
                                   ("rgb8 through InstanceReplayFormat", seq["rgb8"], "rgb8", "replay")):
        got = _run(seq, frames, fmt, how)
        assert got[3] == N, name
        assert got[0] == want, "%s: the output log differs from the gray run's" % name
    want_nv12 = _run(seq, seq["gray_nv12"])
    got = _run(seq, seq["nv12"], ("nv12", 0, 1))             # a whole surface per frame: only the luma rows are read
    assert got[3] == N == want_nv12[3]
    assert got[0] == want_nv12[0], "nv12 + limited_range: the output log differs from the gray run's"


@pytest.mark.parametrize("bad,word", [((99,), "format"), ((-1,), "format"), (("gray16", 7), "bits"), (("gray16", 17), "bits"),
                                      (("rgb8", 0, 1), "limited_range"), (("bgra8", 0, 1), "limited_range")])
def test_cpu_reference_reports_a_bad_format_and_goes_on(seq, bad, word):
    s = runner.Session(ORACLE_LIB, dict(seq, frames=seq["yuyv"]), slam_yaml=BENCH_YAML, pixel_format=bad)
    assert s.step()
    assert "Image format is not supported" in s.error() and word in s.error()
    assert s.times().frames == 0
    s.pixel_format = runner.frame_format("yuyv")            # the library goes on with the next (supported) frame
    assert s.step() and s.step()
    s.flush()
    s.sync()
    assert s.times().frames == 2
    s.close()


def test_cpu_reference_reports_a_short_stride(seq):
    s = runner.Session(ORACLE_LIB, dict(seq, frames=seq["gray"]), slam_yaml=BENCH_YAML, pixel_format="gray16")   # rows of w bytes, 2 w needed
    assert s.step()
    assert "stride" in s.error() and s.times().frames == 0
    s.close()


CALLER = r"""
#include "XRSLAM.h"
#include "xrslam_hip.h"
int call_format(xrhip_image *img, XRSLAMAmdInstance *inst, const void *px, const double *imu7, const double *cam_t, int *cur) {
    XRSLAMAmdFrameFormat f = {XRSLAM_AMD_PIXEL_GRAY16, 10, 0};
    int rc = xrhip_image_upload_format(img, px, 752 * 2, XRHIP_PIXFMT_YUYV, 0, 1, 0);
    rc += xrhip_image_upload_format_distorted(img, px, 752 * 2, XRHIP_PIXFMT_P010, 0, 0, 1);
    XRSLAMAmdPushImageFormat(px, 752 * 2, &f, 1, 0.5);
    XRSLAMAmdInstancePushImageFormat(inst, px, 752 * 2, &f, 0, 0.5);
    return rc + XRSLAMAmdInstanceReplayFormat(inst, imu7, 1, cam_t, 1, px, (size_t)752 * 480 * 2, 752 * 2, &f, 0, cur, cur + 1, 1, 0);
}
int enum_matches[(int)XRSLAM_AMD_PIXEL_P010 == XRHIP_PIXFMT_P010 && (int)XRSLAM_AMD_PIXEL_GRAY16 == XRHIP_PIXFMT_GRAY16 &&
                 (int)XRSLAM_AMD_PIXEL_RGB8 == XRHIP_PIXFMT_RGB8 ? 1 : -1];
"""
NEW_SYMBOLS = ("xrhip_image_upload_format", "xrhip_image_upload_format_distorted", "XRSLAMAmdPushImageFormat",
               "XRSLAMAmdInstancePushImageFormat", "XRSLAMAmdInstanceReplayFormat")


def test_format_entry_points_are_declared_for_c_and_exported(tmp_path):
    """A C caller compiles against include/XRSLAM.h and include/xrslam_hip.h, whose format numbers agree; the product library exports
    what it calls; the CPU reference build exports the outer three and leaves the two inner ones weak and undefined."""
    from xrslam_amd import _lib, abi
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
    assert [getattr(abi, "PIXFMT_" + n.upper()) for n in pm.NAMES] == list(range(11)) == [runner.PIXEL_FORMATS[n] for n in pm.NAMES]
    assert abi.PIXFMT_BYTES == pm.BYTES
