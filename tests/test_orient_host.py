"""The host side of the frame orientation under AddressSanitizer and UBSan: tests/host_check/orient_host.cpp, a stand-alone program
(its own main, no GPU code, never loaded into Python) over xrslam_amd/csrc/host/pixel_format.hpp -- the EXIF table, the host turn of
a build without the device kernel and the intrinsics map with its rotation R, what XRSLAMAmdOrientationFromExif and
XRSLAMAmdOrientIntrinsics hand out -- held against tests/orient_model.py line by line."""
import os
import subprocess

import numpy as np
import pytest

from tests import orient_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "orient_host.cpp")
OUT = os.path.join(ROOT, "tests", "host_check", "_build", "orient_host")
DEPS = [SRC, os.path.join(ROOT, "xrslam_amd", "csrc", "host", "pixel_format.hpp"), os.path.join(ROOT, "include", "xrslam_hip.h")]
K = (458.654, 457.296, 367.215, 248.375)
GEOS = [None, (1920, 1080, 114, 0, 1692, 1080), (1300, 1000, 3, 5, 1111, 977)]
W, H = 752, 480


@pytest.fixture(scope="module")
def lines():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", SRC, "-o", OUT])
    p = subprocess.run([OUT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = p.stdout.strip().splitlines()
    assert out[-1] == "ok"
    return [ln.split() for ln in out[:-1]]


def test_the_exif_table(lines):
    got = {int(ln[1]): int(ln[2]) for ln in lines if ln[0] == "E"}
    assert got == {e: om.from_exif(e) for e in range(-1, 11)}
    assert {e: o for e, o in got.items() if o >= 0} == {1: 0, 6: 1, 3: 2, 8: 3, 2: 4, 7: 5, 4: 6, 5: 7}


def test_the_host_turn_equals_the_model(lines):
    rows = [ln for ln in lines if ln[0] == "P"]
    assert len(rows) == 24
    for ln in rows:
        o, sw, sh = int(ln[1]), int(ln[2]), int(ln[3])
        src = ((17 * np.arange(sw * sh) + 3) % 256).astype(np.uint8).reshape(sh, sw)
        np.testing.assert_array_equal(np.array(ln[4:], dtype=np.int64), om.orient(src, o).reshape(-1), err_msg=" ".join(ln[:4]))


def test_orient_intrinsics_and_its_rotation_equal_the_model(lines):
    rows = [ln for ln in lines if ln[0] == "I"]
    assert len(rows) == 24
    for ln in rows:
        c, o = int(ln[1]), int(ln[2])
        v = np.array(ln[3:], dtype=np.float64)
        Km, R = om.orient_intrinsics(K, GEOS[c], o, W, H)
        np.testing.assert_allclose(v[:4], Km, rtol=0, atol=1e-10, err_msg="case %d, o %d" % (c, o))
        np.testing.assert_array_equal(v[4:].reshape(3, 3), R, err_msg="case %d, o %d" % (c, o))
        assert round(np.linalg.det(R)) == (-1 if o >> 2 else 1)
