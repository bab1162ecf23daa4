"""The optional feature_tracker.lk_* keys through the outer C API, without a GPU: the host pipeline over the CPU reference build
(oracle/_build/libxrslam_oracle.so), a library behind include/xrslam_hip.h WITHOUT xrhip_klt_set_lk_params.  Parsing, what
XRSLAMAmdDescribeConfig prints, invalid values, keys at the reference's values (run, same output log as no keys) and other values
(creation fails with a message that says why)."""
import ctypes as C
import glob
import os
import subprocess
import tempfile

import pytest

from tests import lk_params_yaml as ly
from xrslam_amd.harness import runner, scene

ROOT = ly.ROOT
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "libxrslam_oracle.so")
N = 40
DEFAULT_KEYS = dict(lk_window_size=21, lk_max_level=3, lk_max_iterations=30, lk_epsilon=0.01)


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    if not os.path.exists(ORACLE_LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


@pytest.fixture(scope="module")
def seq():
    return scene.make_sequence(n_frames=N, seed=1, w=320, h=240, K=(195.0, 194.5, 160.0, 120.0))


def _create(slam, sensor=ly.SENSOR_320):
    """XRSLAMCreate on the process-global instance -> (lib, ok, last error)"""
    lib = runner.load(ORACLE_LIB)
    cfg = C.c_void_p()
    ok = lib.XRSLAMCreate(slam.encode(), sensor.encode(), b"", b"xrslam_amd", C.byref(cfg))
    return lib, ok, lib.XRSLAMAmdLastError().decode()


def test_absent_keys_mean_the_reference_constants_and_shipped_configs_describe_as_before(tmp_path):
    """Every shipped slam yaml: no lk line in XRSLAMAmdDescribeConfig, GetTrackerParams reports 21 / 3 / 30 / 0.01; with the four keys
    written at those values the text is the same text plus the four lines."""
    slams = sorted(glob.glob(os.path.join(ROOT, "configs", "*slam*.yaml")))
    assert ly.BENCH_YAML in slams and len(slams) >= 3
    for slam in slams:
        lib, ok, err = _create(slam)
        assert ok == 1, (slam, err)
        text = ly.describe(lib)
        assert "lk_" not in text, slam
        p = ly.TrackerParams()
        lib.XRSLAMAmdGetTrackerParams.argtypes = [C.POINTER(ly.TrackerParams)]
        assert lib.XRSLAMAmdGetTrackerParams(C.byref(p)) == 1
        assert (p.lk_window_size, p.lk_max_level, p.lk_max_iterations, p.lk_epsilon) == (21, 3, 30, 0.01)
        lib.XRSLAMDestroy()
    lib, ok, err = _create(ly.BENCH_YAML)
    plain = ly.describe(lib)
    lib.XRSLAMDestroy()
    lib, ok, err = _create(ly.slam_yaml(tmp_path / "keys.yaml", **DEFAULT_KEYS))
    assert ok == 1, err
    keyed = ly.describe(lib).splitlines()
    lib.XRSLAMDestroy()
    extra = ["feature_tracker.lk_window_size = 21", "feature_tracker.lk_max_level = 3", "feature_tracker.lk_max_iterations = 30",
             "feature_tracker.lk_epsilon = 0.01"]
    assert [ln for ln in keyed if "lk_" in ln] == extra
    assert [ln for ln in keyed if "lk_" not in ln] == plain.splitlines()
    i = keyed.index(extra[0])
    assert keyed[i - 1].startswith("feature_tracker.predict_keypoints") and keyed[i + 4].startswith("initializer.keyframe_num")


def test_a_single_key_is_parsed_and_the_others_keep_their_defaults(tmp_path):
    lib, ok, err = _create(ly.slam_yaml(tmp_path / "eps.yaml", lk_epsilon="0.01   # the reference's"))
    assert ok == 1, err
    assert "feature_tracker.lk_epsilon = 0.01" in ly.describe(lib) and "feature_tracker.lk_window_size = 21" in ly.describe(lib)
    lib.XRSLAMDestroy()


BAD = [
    (dict(lk_window_size=20), "lk_window_size"),
    (dict(lk_window_size=23), "lk_window_size"),
    (dict(lk_window_size=3), "lk_window_size"),
    (dict(lk_window_size=15.5), "lk_window_size"),
    (dict(lk_max_level=6), "lk_max_level"),
    (dict(lk_max_level=-1), "lk_max_level"),
    (dict(lk_window_size=21, lk_max_level=4), "lk_max_level"),        # 320 x 240: level 4 is 20 x 15
    (dict(lk_max_iterations=0), "lk_max_iterations"),
    (dict(lk_max_iterations=101), "lk_max_iterations"),
    (dict(lk_epsilon=-0.1), "lk_epsilon"),
    (dict(lk_epsilon=10.5), "lk_epsilon"),
]


@pytest.mark.parametrize("keys,word", BAD, ids=["_".join("%s%s" % kv for kv in k.items()) for k, _ in BAD])
def test_invalid_values_fail_the_creation_with_a_message(tmp_path, keys, word):
    slam = ly.slam_yaml(tmp_path / "bad.yaml", **keys)
    lib, ok, err = _create(slam)
    assert ok != 1
    assert "feature_tracker." + word in err, err
    handle, cfg = C.c_void_p(), C.c_void_p()
    assert lib.XRSLAMAmdInstanceCreate(slam.encode(), ly.SENSOR_320.encode(), C.byref(handle), C.byref(cfg)) != 1
    assert "feature_tracker." + word in lib.XRSLAMAmdLastError().decode()


@pytest.mark.parametrize("keys", [dict(lk_window_size=15, lk_max_level=2), dict(lk_max_iterations=10), dict(lk_epsilon=0.03)],
                         ids=["window_level", "iterations", "epsilon"])
def test_other_values_fail_cleanly_against_a_library_without_the_entry_point(tmp_path, keys):
    lib, ok, err = _create(ly.slam_yaml(tmp_path / "other.yaml", **keys))
    assert not hasattr(lib, "xrhip_klt_set_lk_params")                     # the CPU reference build is such a library
    assert ok != 1
    assert "xrhip_klt_set_lk_params" in err and "21 / 3 / 30 / 0.01" in err, err
    lib, ok, err = _create(ly.BENCH_YAML)                                  # and the next creation works
    assert ok == 1, err
    lib.XRSLAMDestroy()


def _logged_run(seq, slam):
    fd, path = tempfile.mkstemp(prefix="xr_out_", suffix=".bin")
    os.close(fd)
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path
    try:
        s = runner.Session(ORACLE_LIB, seq, slam_yaml=slam, sensor_yaml=ly.SENSOR_320, instance=True)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    params = ly.tracker_params(s)
    while s.step():
        assert not s.error(), s.error()
    s.flush()
    s.sync()
    assert not s.error(), s.error()
    frames = s.times().frames
    s.close()
    with open(path, "rb") as fh:
        blob = fh.read()
    os.unlink(path)
    return blob, frames, params


def test_keys_at_the_reference_values_run_and_write_the_log_of_no_keys(tmp_path, seq):
    want, frames, params = _logged_run(seq, ly.BENCH_YAML)
    assert frames == N and params == (21, 3, 30, 0.01) and len(want) > 1000
    got, frames2, params2 = _logged_run(seq, ly.slam_yaml(tmp_path / "keys.yaml", **DEFAULT_KEYS))
    assert frames2 == N and params2 == params
    assert got == want
