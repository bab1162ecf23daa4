"""CPU tests of the configuration surface and the error behaviour of the outer C ABI (include/XRSLAM.h), run on the
CPU reference library (the product's host sources linked against the oracle, oracle/_build/libxrslam_oracle.so):
mandatory device keys (yaml_config.cpp:152-212), optional slam keys with the defaults of config.cpp:7-78, and what
XRSLAMCreate reports instead of the reference's uncaught YamlConfig exceptions."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_build", "libxrslam_oracle.so")
SLAM = os.path.join(ROOT, "configs", "euroc_slam.yaml")
SENSOR = os.path.join(ROOT, "configs", "euroc_sensor.yaml")


class Intrinsics(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(REF_LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    from xrslam_amd.harness import runner
    return runner.load(REF_LIB)


def _create(lib, slam, sensor):
    cfg = C.c_void_p()
    ok = lib.XRSLAMCreate(slam.encode(), sensor.encode(), b"", b"test", C.byref(cfg))
    err = lib.XRSLAMAmdLastError().decode()
    return ok, err, cfg


def test_create_with_the_shipped_configuration(lib):
    ok, err, cfg = _create(lib, SLAM, SENSOR)
    assert ok == 1 and cfg.value
    k = Intrinsics()
    lib.XRSLAMGetResult(9, C.byref(k))          # XRSLAM_INFO_INTRINSICS (XRSLAM.h: after the result types and UNKNOWN)
    assert (k.fx, k.fy, k.cx, k.cy) == (458.654, 457.296, 367.215, 248.375)
    lib.XRSLAMDestroy()
    lib.XRSLAMDestroy()                           # idempotent; calls on a destroyed instance are ignored
    lib.XRSLAMRunOneFrame()


def test_missing_files_and_mandatory_keys(lib, tmp_path):
    ok, err, _ = _create(lib, SLAM, str(tmp_path / "nope.yaml"))
    assert ok == 0 and "cannot load config" in err           # YamlConfig::LoadException in the reference
    ok, err, _ = _create(lib, str(tmp_path / "nope.yaml"), SENSOR)
    assert ok == 0 and "cannot load config" in err
    text = open(SENSOR).read()
    # every mandatory device key (yaml_config.cpp:152-212): dropping it is ConfigMissingException there, 0 + message here
    for key, leaf in (("cam0.intrinsics", "intrinsics:"), ("cam0.resolution", "resolution:"), ("imu.noise.cov_g", "cov_g:"),
                      ("cam0.extrinsic.q_bc", "q_bc:"), ("cam0.time_offset", "time_offset:")):
        lines = text.splitlines()
        i = next(n for n, ln in enumerate(lines) if ln.strip().startswith(leaf))
        j = i + 1
        while lines[j - 1].count("[") - lines[j - 1].count("]") + sum(l.count("[") - l.count("]") for l in lines[i:j - 1]) > 0:
            j += 1                                   # a flow sequence may span several lines
        broken = tmp_path / ("no_%s.yaml" % key.replace(".", "_"))
        broken.write_text("\n".join(lines[:i] + lines[j:]) + "\n")
        ok, err, _ = _create(lib, SLAM, str(broken))
        assert ok == 0 and err == "config missing: " + key, (key, err)
    # wrong arity is the reference's TypeErrorException
    bad = tmp_path / "bad_arity.yaml"
    bad.write_text(text.replace("resolution: [752, 480]", "resolution: [752]"))
    assert "resolution: [752]" in bad.read_text()
    ok, err, _ = _create(lib, SLAM, str(bad))
    assert ok == 0 and err == "config type error: cam0.resolution"


def test_slam_keys_are_optional(lib, tmp_path):
    """A slam file without any key is valid: every accessor falls back to config.cpp's default (window 10, 150
    features, CLAHE 6.0 / 8x8, iteration limit 10, ...)."""
    empty = tmp_path / "empty_slam.yaml"
    empty.write_text("%YAML:1.0\n---\n")
    ok, err, _ = _create(lib, str(empty), SENSOR)
    assert ok == 1, err
    assert err == ""                                  # a successful create clears the error of the failed ones above
    lib.XRSLAMDestroy()


# the reference's configs/euroc_slam.yaml and configs/euroc_sensor.yaml, byte for byte (data fixtures)
REF_CFG = os.path.join(ROOT, "tests", "golden", "reference_configs")


def _describe(lib, slam, sensor):
    ok, err, _ = _create(lib, slam, sensor)
    assert ok == 1, err
    lib.XRSLAMAmdDescribeConfig.argtypes = [C.c_char_p, C.c_int]
    lib.XRSLAMAmdDescribeConfig.restype = C.c_int
    n = lib.XRSLAMAmdDescribeConfig(None, 0)
    buf = C.create_string_buffer(n + 1)
    assert lib.XRSLAMAmdDescribeConfig(buf, n + 1) == n
    cam = (C.c_double * 16)()
    lib.XRSLAMAmdGetCameraConfig.argtypes = [C.c_void_p]
    lib.XRSLAMAmdGetCameraConfig.restype = None
    lib.XRSLAMAmdGetCameraConfig(cam)
    lib.XRSLAMDestroy()
    text = buf.value.decode()
    return dict(ln.split(" = ") for ln in text.splitlines()), bytes(cam)


def test_the_reference_yaml_files_load_verbatim_and_mean_the_shipped_configuration(lib):
    """XRSLAMCreate on the reference's configs/euroc_slam.yaml + euroc_sensor.yaml AS SHIPPED BY THE REFERENCE (multi-line flow
    sequences, the nested T_BS map, keys this library does not read): accepted, and every value it resolves to -- all of
    xrslam::Config's accessors (XRSLAMAmdDescribeConfig) and the XRSLAMAmdCameraConfig the dataset readers ask for -- equals what
    the repo's re-formatted copies under configs/ resolve to."""
    ref, ref_cam = _describe(lib, os.path.join(REF_CFG, "euroc_slam.yaml"), os.path.join(REF_CFG, "euroc_sensor.yaml"))
    ours, our_cam = _describe(lib, SLAM, SENSOR)
    assert ref == ours
    assert ref_cam == our_cam
    assert len(ref) == 44
    # spot values straight from the reference's files (configs/euroc_slam.yaml:6-36, euroc_sensor.yaml:40-53)
    assert ref["sliding_window.size"] == "10" and ref["feature_tracker.max_keypoint_detection"] == "200"
    assert ref["solver.iteration_limit"] == "30" and ref["rotation.misalignment_threshold"] == "0.02"
    assert ref["cam0.intrinsics"] == "458.654 457.29599999999999 367.21499999999997 248.375"
    assert ref["cam0.resolution"] == "752 480" and ref["cam0.noise"] == "0.5 0 0 0.5"


def test_describe_config_reports_defaults_for_an_empty_slam_file(lib, tmp_path):
    empty = tmp_path / "empty_slam.yaml"
    empty.write_text("%YAML:1.0\n---\n")
    d, _ = _describe(lib, str(empty), SENSOR)
    # config.cpp:7-78
    assert d["sliding_window.size"] == "10" and d["feature_tracker.max_keypoint_detection"] == "150"
    assert d["solver.iteration_limit"] == "10" and d["rotation.misalignment_threshold"] == "0.10000000000000001"
    assert d["feature_tracker.max_init_frames"] == "60" and d["initializer.keyframe_num"] == "8"
