"""The mask entry points without a GPU: the symbols, their argument errors, and the player's --mask loader.

tests/host_check/mask_host.cpp is a stand-alone program (its own main, no GPU code, never loaded into Python) built with
AddressSanitizer and UBSan over xrslam_amd/csrc/player/euroc_io.hpp: it loads the mask files written here, each read into a heap block
of exactly the file's size, and prints a checksum of the pixels or the loader's error.

The outer API is driven over the CPU reference build (oracle/_build/libxrslam_oracle.so: the host pipeline over a library behind
include/xrslam_hip.h WITHOUT the mask entry points -- masks for the CPU-reference pipeline are out of scope): clearing a mask that
was never set is a no-op, a bad stride and a mask the library cannot take are refused with a reason, and nothing aborts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from xrslam_amd import _lib
from xrslam_amd._lib import XRHIP_EINVAL
from xrslam_amd.harness import runner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "mask_host.cpp")
OUT = os.path.join(ROOT, "tests", "host_check", "_build", "mask_host")
DEPS = [SRC, os.path.join(ROOT, "xrslam_amd", "csrc", "player", "euroc_io.hpp")]
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "libxrslam_oracle.so")
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR_320 = os.path.join(ROOT, "tests", "golden", "small_sensor_320.yaml")
W, H = 320, 240


def fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_symbols_are_exported_and_refuse_null_arguments():
    lib = _lib.lib()
    vp = C.c_void_p
    for name in ("xrhip_klt_set_mask", "xrhip_image_set_mask"):
        fn = getattr(lib, name)
        fn.argtypes = [vp, vp, C.c_int, C.c_int]
        buf = np.ones(16, np.uint8)
        assert fn(None, buf.ctypes.data, 4, 0) == XRHIP_EINVAL
        assert name.encode() in lib.xrhip_last_error()
        assert fn(None, None, 0, 0) == XRHIP_EINVAL
    lib.xrhip_debug_get_mask.argtypes = [vp, vp]
    assert lib.xrhip_debug_get_mask(None, None) == XRHIP_EINVAL
    assert b"xrhip_debug_get_mask" in lib.xrhip_last_error()
    # the outer entry points: no instance -> 0 with a reason
    out = runner.load(_lib.LIB_PATH)
    for name in ("XRSLAMAmdSetMask", "XRSLAMAmdSetNextFrameMask"):
        assert getattr(out, name)(None, 0, 0) == 0
        assert b"no instance" in out.XRSLAMAmdLastError()
    for name in ("XRSLAMAmdInstanceSetMask", "XRSLAMAmdInstanceSetNextFrameMask"):
        assert getattr(out, name)(None, None, 0, 0) == 0


CALLER = r"""
#include "XRSLAM.h"
#include "xrslam_hip.h"
int (*a)(xrhip_klt *, const void *, int, int) = xrhip_klt_set_mask;
int (*b)(xrhip_image *, const void *, int, int) = xrhip_image_set_mask;
int (*c)(xrhip_image *, uint8_t *) = xrhip_debug_get_mask;
int (*d)(const void *, int, int) = XRSLAMAmdSetMask;
int (*e)(const void *, int, int) = XRSLAMAmdSetNextFrameMask;
int (*f)(XRSLAMAmdInstance *, const void *, int, int) = XRSLAMAmdInstanceSetMask;
int (*g)(XRSLAMAmdInstance *, const void *, int, int) = XRSLAMAmdInstanceSetNextFrameMask;
"""


def test_the_headers_declare_them_for_c_and_cxx(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++17")):
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I" + os.path.join(ROOT, "include"), "-c",
                               str(src), "-o", str(tmp_path / ("caller_%s.o" % cc))])


def test_python_mask_arguments():
    from xrslam_amd import abi
    m = np.ones((H, W + 8), np.uint8)[:, :W]
    ptr, stride = abi.mask_args(m, W, H)
    assert ptr.value == m.ctypes.data and stride == W + 8
    assert abi.mask_args(None, W, H) == (None, 0)
    ptr, stride = abi.mask_args(0x1001, W, H, on_device=True, stride=333)
    assert ptr.value == 0x1001 and stride == 333
    with pytest.raises(AssertionError):
        abi.mask_args(np.ones((H, W + 1), np.uint8), W, H)


def test_outer_api_over_the_cpu_reference_build():
    if not os.path.exists(ORACLE_LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    lib = runner.load(ORACLE_LIB)
    cfg = C.c_void_p()
    assert lib.XRSLAMCreate(BENCH_YAML.encode(), SENSOR_320.encode(), b"", b"xrslam_amd", C.byref(cfg)) == 1
    try:
        assert lib.XRSLAMAmdLastError() == b""
        assert lib.XRSLAMAmdSetMask(None, 0, 0) == 1              # nothing set: clearing is a no-op
        assert lib.XRSLAMAmdSetNextFrameMask(None, 0, 0) == 1
        assert lib.XRSLAMAmdLastError() == b""
        m = np.ones((H, W), np.uint8)
        for fn in (lib.XRSLAMAmdSetMask, lib.XRSLAMAmdSetNextFrameMask):
            assert fn(m.ctypes.data, W - 1, 0) == 0
            assert b"stride" in lib.XRSLAMAmdLastError()
            assert fn(m.ctypes.data, W, 0) == 0                   # (this build has no masks: refused, with the reason)
            assert b"not supported" in lib.XRSLAMAmdLastError()
    finally:
        lib.XRSLAMDestroy()


def pgm(mask, header=None):
    h, w = mask.shape
    return (header or b"P5\n%d %d\n255\n" % (w, h)) + mask.tobytes()


def test_the_players_mask_loader_is_right_and_clean_under_the_sanitizers(tmp_path):
    from PIL import Image
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", SRC, "-o", OUT, "-lz"])
    m = np.random.RandomState(4).choice(np.array([0, 1, 128, 255], np.uint8), size=(H, W))
    small = m[:100, :200].copy()
    files = {
        "good.pgm": pgm(m),
        "comment.pgm": pgm(m, b"P5 # a mask\n# made by hand\n%d\t%d\n255\n" % (W, H)),
        "small.pgm": pgm(small),
        "short.pgm": pgm(m)[:-1],
        "wide.pgm": pgm(m, b"P5\n%d %d\n65535\n" % (W, H)),
        "ascii.pgm": b"P2\n2 2\n255\n0 1 2 3\n",
        "nospace.pgm": b"P5\n2 2\n255",
        "huge.pgm": b"P5\n99999 99999\n255\n",
        "empty.pgm": b"",
    }
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    Image.fromarray(m).save(str(tmp_path / "good.png"))
    Image.fromarray(small).save(str(tmp_path / "small.png"))
    names = list(files) + ["good.png", "small.png"]
    p = subprocess.run([OUT, str(W), str(H)] + [str(tmp_path / n) for n in names], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = dict(zip(names, p.stdout.strip().splitlines()))
    assert len(got) == len(names)
    ok = "ok %d %d %016x %d" % (W, H, fnv1a(m.tobytes()), int((m != 0).sum()))
    assert got["good.pgm"] == ok and got["comment.pgm"] == ok and got["good.png"] == ok
    for n in ("small.pgm", "small.png"):   # a size mismatch names both sizes
        assert got[n] == "error mask: the file is 200 x 100, the working resolution is 320 x 240", got[n]
    assert "shorter" in got["short.pgm"] and "maxval" in got["wide.pgm"] and "bad size" in got["huge.pgm"]
    for n in ("ascii.pgm", "nospace.pgm", "empty.pgm"):
        assert got[n].startswith("error "), (n, got[n])
