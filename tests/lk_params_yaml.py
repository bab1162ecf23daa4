"""A slam yaml with the optional feature_tracker.lk_* keys added to configs/bench_slam_150.yaml, and the outer API's view of them."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR_320 = os.path.join(ROOT, "tests", "golden", "small_sensor_320.yaml")
KEYS = ("lk_window_size", "lk_max_level", "lk_max_iterations", "lk_epsilon")


def slam_yaml(path, base=BENCH_YAML, **keys):
    """Writes `base` with the given feature_tracker.lk_* keys (raw yaml scalars) at the end of its feature_tracker block -> path"""
    assert set(keys) <= set(KEYS), keys
    text = open(base).read()
    anchor = "  clahe_height: 8\n"
    assert text.count(anchor) == 1
    text = text.replace(anchor, anchor + "".join("  %s: %s\n" % (k, keys[k]) for k in KEYS if k in keys))
    with open(path, "w") as fh:
        fh.write(text)
    return str(path)


class TrackerParams(C.Structure):   # XRSLAMAmdTrackerParams (include/XRSLAM.h)
    _fields_ = [("lk_window_size", C.c_int), ("lk_max_level", C.c_int), ("lk_max_iterations", C.c_int), ("lk_epsilon", C.c_double)]


def tracker_params(session):
    """(window, max_level, iterations, epsilon) of a runner.Session, through the global or the instance entry point"""
    p = TrackerParams()
    h = getattr(session, "_handle", None)
    if h is None:
        fn = session.lib.XRSLAMAmdGetTrackerParams
        fn.argtypes = [C.POINTER(TrackerParams)]
        assert fn(C.byref(p)) == 1
    else:
        fn = session.lib.XRSLAMAmdInstanceGetTrackerParams
        fn.argtypes = [C.c_void_p, C.POINTER(TrackerParams)]
        assert fn(h, C.byref(p)) == 1
    return p.lk_window_size, p.lk_max_level, p.lk_max_iterations, p.lk_epsilon


def describe(lib):
    """XRSLAMAmdDescribeConfig of the process-global instance -> text"""
    lib.XRSLAMAmdDescribeConfig.argtypes = [C.c_char_p, C.c_int]
    lib.XRSLAMAmdDescribeConfig.restype = C.c_int
    n = lib.XRSLAMAmdDescribeConfig(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.XRSLAMAmdDescribeConfig(buf, n + 1)
    return buf.value.decode()
