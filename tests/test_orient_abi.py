"""The outer C ABI's orientation helpers and its sticky setting (include/XRSLAM.h: XRSLAMAmdOrientationFromExif,
XRSLAMAmdOrientIntrinsics, XRSLAMAmdSetFrameOrientation / GetFrameOrientation) through the built library, against
tests/orient_model.py.  Pure host code behind these entry points: no GPU, no instance."""
import ctypes as C

import numpy as np

from tests import orient_model as om

ORIENTATIONS = tuple(range(8))


def test_the_librarys_helpers_equal_the_model():
    from xrslam_amd import _lib
    from xrslam_amd.harness import runner
    lib = runner.load(_lib.LIB_PATH)
    assert [lib.XRSLAMAmdOrientationFromExif(e) for e in range(-1, 11)] == [om.from_exif(e) for e in range(-1, 11)]
    W, H = 752, 480
    K = np.array((458.654, 457.296, 367.215, 248.375))
    for geo in (None, (1920, 1080, 114, 0, 1692, 1080), (1300, 1000, 3, 5, 1111, 977)):
        g = C.byref(runner.frame_geometry(geo)) if geo is not None else None
        for o in ORIENTATIONS:
            out, R = np.zeros(4), np.zeros(9)
            assert lib.XRSLAMAmdOrientIntrinsics(K.ctypes.data, g, o, W, H, out.ctypes.data, R.ctypes.data) == 1
            Km, Rm = om.orient_intrinsics(K, geo, o, W, H)
            np.testing.assert_allclose(out, Km, rtol=0, atol=1e-10)
            np.testing.assert_array_equal(R.reshape(3, 3), Rm)
    out, R = np.full(4, 7.0), np.full(9, 7.0)
    for bad in (8, -1):
        assert lib.XRSLAMAmdOrientIntrinsics(K.ctypes.data, None, bad, W, H, out.ctypes.data, R.ctypes.data) == 0
    assert lib.XRSLAMAmdOrientIntrinsics(None, None, 1, W, H, out.ctypes.data, R.ctypes.data) == 0
    assert (out == 7).all() and (R == 7).all()


def test_the_process_global_setting_keeps_its_value_through_a_bad_one():
    """Whatever an earlier test of the process left behind: the value set here is read back, a bad value is reported and changes
    nothing, and the setting is put back as it was found."""
    from xrslam_amd import _lib
    from xrslam_amd.harness import runner
    lib = runner.load(_lib.LIB_PATH)
    found = lib.XRSLAMAmdGetFrameOrientation()
    assert 0 <= found <= 7
    try:
        for o in (5, 0, 3):
            assert lib.XRSLAMAmdSetFrameOrientation(o) == 1 and lib.XRSLAMAmdGetFrameOrientation() == o
            for bad in (8, -1):
                assert lib.XRSLAMAmdSetFrameOrientation(bad) == 0 and b"orientation" in lib.XRSLAMAmdLastError()
                assert lib.XRSLAMAmdGetFrameOrientation() == o
    finally:
        assert lib.XRSLAMAmdSetFrameOrientation(found) == 1
