"""The player's call sequence (reference xrslam-pc/player/src/main.cpp:116-169) over the outer C ABI
(include/XRSLAM.h): at equal timestamps the asynchronous dataset reader yields gyroscope, then
accelerometer, then camera (IO/async_dataset_reader.cpp:41-48).  Works against any shared object that
exports the XRSLAM.h symbols (the product library, or the oracle-backed CPU reference build)."""
import ctypes as C
import os

import numpy as np

XRSLAM_SENSOR_CAMERA, XRSLAM_SENSOR_ACCELERATION, XRSLAM_SENSOR_GYROSCOPE = 0, 2, 3
XRSLAM_RESULT_BODY_POSE, XRSLAM_RESULT_STATE = 0, 2


class XRSLAMImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("timeStamp", C.c_double), ("stride", C.c_int), ("camera_id", C.c_int),
                ("channel", C.c_int), ("ext", C.c_void_p)]


class XRSLAMVec3(C.Structure):       # XRSLAMAcceleration / XRSLAMGyroscope
    _fields_ = [("data", C.c_double * 3), ("timestamp", C.c_double)]


class XRSLAMPose(C.Structure):
    _fields_ = [("quaternion", C.c_double * 4), ("translation", C.c_double * 3), ("timestamp", C.c_double)]


class BaStats(C.Structure):   # xrhip_ba_stats (include/xrslam_hip.h)
    _fields_ = [("n_solve_try", C.c_long), ("n_trials", C.c_long), ("ms_solve_try", C.c_double), ("n_timed", C.c_long),
                ("flops_solve_try", C.c_double), ("n_tiny", C.c_long), ("n_chain_timed", C.c_long), ("ms_chain", C.c_double),
                ("bytes_chain", C.c_double), ("n_cov_launches", C.c_long)]


class XRSLAMAmdCovariance(C.Structure):   # include/XRSLAM.h
    _fields_ = [("timestamp", C.c_double), ("state", (C.c_double * 15) * 15), ("pose_ros", (C.c_double * 6) * 6), ("status", C.c_int),
                ("rcond_estimate", C.c_double)]


class XRSLAMAmdTimes(C.Structure):
    _fields_ = [("frames", C.c_long), ("solves", C.c_long), ("solve_iterations", C.c_long),
                ("marginalizations", C.c_long), ("keyframes", C.c_long), ("ba_device_ms", C.c_double),
                ("wall_preprocess", C.c_double), ("wall_track", C.c_double), ("wall_detect", C.c_double),
                ("wall_preintegrate", C.c_double), ("wall_solve", C.c_double), ("wall_marginalize", C.c_double),
                ("wall_frame", C.c_double), ("wall_scope", C.c_double * 16)]


class XRSLAMAmdFeature(C.Structure):   # include/XRSLAM.h
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("track_id", C.c_longlong), ("age", C.c_int), ("n_trail", C.c_int),
                ("trail", (C.c_double * 2) * 8)]


class XRSLAMAmdViewOptions(C.Structure):
    _fields_ = [("color_mode", C.c_int), ("draw_new", C.c_int), ("trail", C.c_int)]


FEATURE_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("track_id", "<i8"), ("age", "<i4"), ("n_trail", "<i4"), ("trail", "<f8", (8, 2))])
assert FEATURE_DTYPE.itemsize == C.sizeof(XRSLAMAmdFeature)


class GroupStats(C.Structure):   # xrhip_group_stats (include/xrslam_hip.h)
    _fields_ = [("batches", C.c_longlong * 12), ("entries", C.c_longlong * 12), ("ms", C.c_double * 12), ("timed", C.c_longlong * 12)]


GROUP_KINDS = ("call", "upload", "preprocess", "track", "detect", "chain", "preint", "window_round", "window_trials", None, None, "gate")   # gate: openings / all present / timeouts


class XRSLAMAmdFrameFormat(C.Structure):
    _fields_ = [("format", C.c_int), ("bits", C.c_int), ("limited_range", C.c_int)]


# XRSLAMAmdPixelFormat (include/XRSLAM.h)
PIXEL_FORMATS = {name: i for i, name in enumerate(("gray8", "bgr8", "bgra8", "rgb8", "rgba8", "gray16", "yuyv", "uyvy", "nv12", "i420",
                                                   "p010"))}
PIXEL_FORMATS.update({name: 16 + i for i, name in enumerate(("bayer_rggb8", "bayer_grbg8", "bayer_gbrg8", "bayer_bggr8", "bayer_rggb16",
                                                             "bayer_grbg16", "bayer_gbrg16", "bayer_bggr16"))})   # (11..15 are not formats)
# packed 10 / 12-bit samples, in a table of their own: gray* = 32 + packing, bayer_* = 40 + 4 * packing + pattern
_PACKINGS = ("10_mipi", "12_mipi", "10p", "12p")
PACKED_PIXEL_FORMATS = {"gray" + pk: 32 + p for p, pk in enumerate(_PACKINGS)}
PACKED_PIXEL_FORMATS.update({"bayer_%s%s" % (pat, pk): 40 + 4 * p + k for p, pk in enumerate(_PACKINGS)
                             for k, pat in enumerate(("rggb", "grbg", "gbrg", "bggr"))})


def frame_format(pixel_format):
    """'yuyv', ('gray16', 10), ('nv12', 0, 1), 'bayer_grbg8', ('bayer_rggb16', 12), 'gray10_mipi' or numbers in their place -> XRSLAMAmdFrameFormat (format, bits, limited_range)"""
    if isinstance(pixel_format, XRSLAMAmdFrameFormat):
        return pixel_format
    f = tuple(pixel_format) if isinstance(pixel_format, (tuple, list)) else (pixel_format,)
    f = f + (0,) * (3 - len(f))
    return XRSLAMAmdFrameFormat((PIXEL_FORMATS[f[0]] if f[0] in PIXEL_FORMATS else PACKED_PIXEL_FORMATS[f[0]]) if isinstance(f[0], str) else int(f[0]), int(f[1]), int(f[2]))


class XRSLAMAmdFrameGeometry(C.Structure):
    _fields_ = [("src_width", C.c_int), ("src_height", C.c_int), ("crop_x", C.c_int), ("crop_y", C.c_int), ("crop_width", C.c_int),
                ("crop_height", C.c_int)]


def frame_geometry(geo):
    """(src_width, src_height, crop_x, crop_y, crop_width, crop_height) -> XRSLAMAmdFrameGeometry"""
    return geo if isinstance(geo, XRSLAMAmdFrameGeometry) else XRSLAMAmdFrameGeometry(*[int(v) for v in geo])


class XRSLAMAmdInitReport(C.Structure):
    _fields_ = [("attempts", C.c_long), ("successes", C.c_long), ("sfm_candidate", C.c_int),
                ("sfm_triangulated", C.c_int), ("scale", C.c_double), ("gravity", C.c_double * 3),
                ("bg", C.c_double * 3)]


ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SLAM_YAML = os.path.join(ROOT, "configs", "euroc_slam.yaml")
SENSOR_YAML = os.path.join(ROOT, "configs", "euroc_sensor.yaml")


def load(lib_path):
    lib = C.CDLL(lib_path)
    lib.XRSLAMCreate.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.XRSLAMPushSensorData.argtypes = [C.c_int, C.c_void_p]
    lib.XRSLAMPushSensorData.restype = None
    lib.XRSLAMRunOneFrame.restype = None
    lib.XRSLAMGetResult.argtypes = [C.c_int, C.c_void_p]
    lib.XRSLAMGetResult.restype = None
    lib.XRSLAMDestroy.restype = None
    lib.XRSLAMAmdSetInitialState.argtypes = [C.c_double] + [C.c_void_p] * 5
    lib.XRSLAMAmdSetInitialState.restype = None
    lib.XRSLAMAmdPushImageDevice.argtypes = [C.c_void_p, C.c_int, C.c_double]
    lib.XRSLAMAmdPushImageDevice.restype = None
    if hasattr(lib, "XRSLAMAmdPushImageDeviceColor"):
        lib.XRSLAMAmdPushImageDeviceColor.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
        lib.XRSLAMAmdPushImageDeviceColor.restype = None
    have_format = hasattr(lib, "XRSLAMAmdPushImageFormat")
    if have_format:
        lib.XRSLAMAmdPushImageFormat.argtypes = [C.c_void_p, C.c_int, C.POINTER(XRSLAMAmdFrameFormat), C.c_int, C.c_double]
        lib.XRSLAMAmdPushImageFormat.restype = None
    have_scaled = hasattr(lib, "XRSLAMAmdPushImageScaled")
    if have_scaled:
        lib.XRSLAMAmdPushImageScaled.argtypes = [C.c_void_p, C.c_int, C.POINTER(XRSLAMAmdFrameFormat), C.POINTER(XRSLAMAmdFrameGeometry),
                                                 C.c_int, C.c_double]
        lib.XRSLAMAmdPushImageScaled.restype = None
        lib.XRSLAMAmdScaleIntrinsics.argtypes = [C.c_void_p, C.POINTER(XRSLAMAmdFrameGeometry), C.c_int, C.c_int, C.c_void_p]
        lib.XRSLAMAmdScaleIntrinsics.restype = None
    have_orient = hasattr(lib, "XRSLAMAmdSetFrameOrientation")
    if have_orient:   # turned / mirrored frames
        lib.XRSLAMAmdSetFrameOrientation.argtypes = [C.c_int]
        lib.XRSLAMAmdGetFrameOrientation.argtypes = []
        lib.XRSLAMAmdOrientationFromExif.argtypes = [C.c_int]
        lib.XRSLAMAmdOrientIntrinsics.argtypes = [C.c_void_p, C.POINTER(XRSLAMAmdFrameGeometry), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.XRSLAMAmdGetTimes.argtypes = [C.POINTER(XRSLAMAmdTimes)]
    lib.XRSLAMAmdGetTimes.restype = None
    lib.XRSLAMAmdLastError.restype = C.c_char_p
    lib.XRSLAMAmdGetInitReport.argtypes = [C.POINTER(XRSLAMAmdInitReport)]
    lib.XRSLAMAmdGetInitReport.restype = None
    lib.XRSLAMAmdSetProfiling.argtypes = [C.c_int]
    lib.XRSLAMAmdSetProfiling.restype = None
    lib.XRSLAMAmdGetKltStats.argtypes = [C.c_void_p, C.c_int]
    lib.XRSLAMAmdGetKltStats.restype = None
    lib.XRSLAMAmdGetBaStats.argtypes = [C.c_void_p, C.c_int]
    lib.XRSLAMAmdGetBaStats.restype = None
    if hasattr(lib, "XRSLAMAmdSetDeviceUndistort"):
        lib.XRSLAMAmdSetDeviceUndistort.argtypes = [C.c_char_p]
        lib.XRSLAMAmdSetDeviceUndistort.restype = None
    lib.XRSLAMAmdSetThreading.argtypes = [C.c_int]
    lib.XRSLAMAmdSetThreading.restype = None
    lib.XRSLAMAmdFlush.restype = None
    have_mask = hasattr(lib, "XRSLAMAmdSetMask")
    if have_mask:   # static / per-frame masks
        lib.XRSLAMAmdSetMask.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.XRSLAMAmdSetNextFrameMask.argtypes = [C.c_void_p, C.c_int, C.c_int]
    have_cov = hasattr(lib, "XRSLAMAmdGetCovariance")
    if have_cov:   # covariance of the newest keyframe / landmark variances
        lib.XRSLAMAmdSetCovariance.argtypes = [C.c_int]
        lib.XRSLAMAmdSetCovariance.restype = None
        lib.XRSLAMAmdGetCovariance.argtypes = [C.POINTER(XRSLAMAmdCovariance)]
        lib.XRSLAMAmdGetLandmarkVariances.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    have_view = hasattr(lib, "XRSLAMAmdRenderTrackingView")
    if have_view:   # the tracking view (feature snapshot + rendered overlay)
        lib.XRSLAMAmdGetFeatures.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        lib.XRSLAMAmdSetFeatureHistory.argtypes = [C.c_int]
        lib.XRSLAMAmdSetFeatureHistory.restype = None
        lib.XRSLAMAmdRenderTrackingView.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(XRSLAMAmdViewOptions)]
    if hasattr(lib, "XRSLAMAmdInstanceCreate"):   # instance-scoped forms: the instance handle is the first argument
        H = C.c_void_p
        lib.XRSLAMAmdInstanceCreate.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(H), C.POINTER(C.c_void_p)]
        for name, args, res in (("Destroy", [], None), ("PushSensorData", [C.c_int, C.c_void_p], None),
                                ("RunOneFrame", [], None), ("GetResult", [C.c_int, C.c_void_p], None),
                                ("SetInitialState", [C.c_double] + [C.c_void_p] * 5, None),
                                ("PushImageDevice", [C.c_void_p, C.c_int, C.c_double], None),
                                ("GetTimes", [C.POINTER(XRSLAMAmdTimes)], None), ("SetProfiling", [C.c_int], None),
                                ("GetBaStats", [C.c_void_p, C.c_int], None), ("GetKltStats", [C.c_void_p, C.c_int], None),
                                ("GetInitReport", [C.POINTER(XRSLAMAmdInitReport)], None), ("LastError", [], C.c_char_p),
                                ("SetDeviceUndistort", [C.c_char_p], None), ("SetThreading", [C.c_int], None),
                                ("Flush", [], None)):
            fn = getattr(lib, "XRSLAMAmdInstance" + name)
            fn.argtypes = [H] + args
            fn.restype = res
        if have_cov:
            lib.XRSLAMAmdInstanceSetCovariance.argtypes = [H, C.c_int]
            lib.XRSLAMAmdInstanceSetCovariance.restype = None
            lib.XRSLAMAmdInstanceGetCovariance.argtypes = [H, C.POINTER(XRSLAMAmdCovariance)]
            lib.XRSLAMAmdInstanceGetLandmarkVariances.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int]
        if have_orient:
            lib.XRSLAMAmdInstanceSetFrameOrientation.argtypes = [H, C.c_int]
            lib.XRSLAMAmdInstanceGetFrameOrientation.argtypes = [H]
        if have_mask:
            lib.XRSLAMAmdInstanceSetMask.argtypes = [H, C.c_void_p, C.c_int, C.c_int]
            lib.XRSLAMAmdInstanceSetNextFrameMask.argtypes = [H, C.c_void_p, C.c_int, C.c_int]
        if have_view:
            lib.XRSLAMAmdInstanceGetFeatures.argtypes = [H, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
            lib.XRSLAMAmdInstanceSetFeatureHistory.argtypes = [H, C.c_int]
            lib.XRSLAMAmdInstanceSetFeatureHistory.restype = None
            lib.XRSLAMAmdInstanceRenderTrackingView.argtypes = [H, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(XRSLAMAmdViewOptions)]
        lib.XRSLAMAmdInstanceReplay.argtypes = [H, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                                C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p]
        lib.XRSLAMAmdInstanceReplay.restype = C.c_int
        if hasattr(lib, "XRSLAMAmdInstanceReplayColor"):
            lib.XRSLAMAmdInstancePushImageDeviceColor.argtypes = [H, C.c_void_p, C.c_int, C.c_int, C.c_double]
            lib.XRSLAMAmdInstancePushImageDeviceColor.restype = None
            lib.XRSLAMAmdInstanceReplayColor.argtypes = [H, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int,
                                                         C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p]
            lib.XRSLAMAmdInstanceReplayColor.restype = C.c_int
        if have_format:
            lib.XRSLAMAmdInstancePushImageFormat.argtypes = [H, C.c_void_p, C.c_int, C.POINTER(XRSLAMAmdFrameFormat), C.c_int, C.c_double]
            lib.XRSLAMAmdInstancePushImageFormat.restype = None
            lib.XRSLAMAmdInstanceReplayFormat.argtypes = [H, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int,
                                                          C.POINTER(XRSLAMAmdFrameFormat), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                          C.c_int, C.c_void_p]
            lib.XRSLAMAmdInstanceReplayFormat.restype = C.c_int
        if have_scaled:
            lib.XRSLAMAmdInstancePushImageScaled.argtypes = [H, C.c_void_p, C.c_int, C.POINTER(XRSLAMAmdFrameFormat),
                                                             C.POINTER(XRSLAMAmdFrameGeometry), C.c_int, C.c_double]
            lib.XRSLAMAmdInstancePushImageScaled.restype = None
            lib.XRSLAMAmdInstanceReplayScaled.argtypes = [H, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int,
                                                          C.POINTER(XRSLAMAmdFrameFormat), C.POINTER(XRSLAMAmdFrameGeometry), C.c_int,
                                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p]
            lib.XRSLAMAmdInstanceReplayScaled.restype = C.c_int
    if hasattr(lib, "XRSLAMAmdGroupCreate"):
        lib.XRSLAMAmdGroupCreate.argtypes = [C.POINTER(C.c_void_p)]
        lib.XRSLAMAmdGroupDestroy.argtypes = [C.c_void_p]
        lib.XRSLAMAmdInstanceJoinGroup.argtypes = [C.c_void_p, C.c_void_p]
        lib.XRSLAMAmdGroupSetProfiling.argtypes = [C.c_void_p, C.c_int]
        lib.XRSLAMAmdGroupSetProfiling.restype = None
        lib.XRSLAMAmdGroupGetStats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.XRSLAMAmdGroupGetStats.restype = None
    return lib


class Group:
    """An instance group (XRSLAMAmdGroup, include/XRSLAM.h): the sessions created with group=<this> share their per-frame launches."""

    def __init__(self, lib_path):
        self.lib = load(lib_path)
        self.handle = C.c_void_p()
        if self.lib.XRSLAMAmdGroupCreate(C.byref(self.handle)) != 1:
            raise RuntimeError("XRSLAMAmdGroupCreate failed: %s" % self.lib.XRSLAMAmdLastError().decode())

    def set_profiling(self, on):
        self.lib.XRSLAMAmdGroupSetProfiling(self.handle, 1 if on else 0)

    def stats(self, reset=False):
        """-> {kind: {"batches", "requests", "ms", "timed"}} for the kinds that saw traffic"""
        st = GroupStats()
        self.lib.XRSLAMAmdGroupGetStats(self.handle, C.byref(st), 1 if reset else 0)
        return {name: {"batches": int(st.batches[i]), "requests": int(st.entries[i]), "ms": float(st.ms[i]), "timed": int(st.timed[i])}
                for i, name in enumerate(GROUP_KINDS) if name and st.batches[i]}

    def close(self):
        if self.handle:
            if self.lib.XRSLAMAmdGroupDestroy(self.handle) != 1:
                raise RuntimeError("XRSLAMAmdGroupDestroy failed: %s" % self.lib.XRSLAMAmdLastError().decode())
            self.handle = None


class _Api:
    """The entry points a Session drives: the process-global ones (the reference's six symbols + XRSLAMAmd*), or their
    XRSLAMAmdInstance* forms bound to one instance handle."""

    def __init__(self, lib, handle=None):
        import functools
        names = {"push": ("XRSLAMPushSensorData", "XRSLAMAmdInstancePushSensorData"),
                 "run": ("XRSLAMRunOneFrame", "XRSLAMAmdInstanceRunOneFrame"),
                 "get_result": ("XRSLAMGetResult", "XRSLAMAmdInstanceGetResult"),
                 "destroy": ("XRSLAMDestroy", "XRSLAMAmdInstanceDestroy"),
                 "set_initial_state": ("XRSLAMAmdSetInitialState", "XRSLAMAmdInstanceSetInitialState"),
                 "push_image_device": ("XRSLAMAmdPushImageDevice", "XRSLAMAmdInstancePushImageDevice"),
                 "get_times": ("XRSLAMAmdGetTimes", "XRSLAMAmdInstanceGetTimes"),
                 "set_profiling": ("XRSLAMAmdSetProfiling", "XRSLAMAmdInstanceSetProfiling"),
                 "get_ba_stats": ("XRSLAMAmdGetBaStats", "XRSLAMAmdInstanceGetBaStats"),
                 "get_klt_stats": ("XRSLAMAmdGetKltStats", "XRSLAMAmdInstanceGetKltStats"),
                 "get_init_report": ("XRSLAMAmdGetInitReport", "XRSLAMAmdInstanceGetInitReport"),
                 "last_error": ("XRSLAMAmdLastError", "XRSLAMAmdInstanceLastError"),
                 "set_device_undistort": ("XRSLAMAmdSetDeviceUndistort", "XRSLAMAmdInstanceSetDeviceUndistort"),
                 "set_threading": ("XRSLAMAmdSetThreading", "XRSLAMAmdInstanceSetThreading"),
                 "sync": ("XRSLAMAmdFlush", "XRSLAMAmdInstanceFlush")}
        if hasattr(lib, "XRSLAMAmdPushImageDeviceColor"):
            names["push_image_device_color"] = ("XRSLAMAmdPushImageDeviceColor", "XRSLAMAmdInstancePushImageDeviceColor")
        if hasattr(lib, "XRSLAMAmdPushImageFormat"):
            names["push_image_format"] = ("XRSLAMAmdPushImageFormat", "XRSLAMAmdInstancePushImageFormat")
        if hasattr(lib, "XRSLAMAmdPushImageScaled"):
            names["push_image_scaled"] = ("XRSLAMAmdPushImageScaled", "XRSLAMAmdInstancePushImageScaled")
        if hasattr(lib, "XRSLAMAmdSetFrameOrientation"):
            names["set_frame_orientation"] = ("XRSLAMAmdSetFrameOrientation", "XRSLAMAmdInstanceSetFrameOrientation")
            names["get_frame_orientation"] = ("XRSLAMAmdGetFrameOrientation", "XRSLAMAmdInstanceGetFrameOrientation")
        if hasattr(lib, "XRSLAMAmdGetCovariance"):
            names["set_covariance"] = ("XRSLAMAmdSetCovariance", "XRSLAMAmdInstanceSetCovariance")
            names["get_covariance"] = ("XRSLAMAmdGetCovariance", "XRSLAMAmdInstanceGetCovariance")
            names["get_landmark_variances"] = ("XRSLAMAmdGetLandmarkVariances", "XRSLAMAmdInstanceGetLandmarkVariances")
        if hasattr(lib, "XRSLAMAmdSetMask"):
            names["set_mask"] = ("XRSLAMAmdSetMask", "XRSLAMAmdInstanceSetMask")
            names["set_next_frame_mask"] = ("XRSLAMAmdSetNextFrameMask", "XRSLAMAmdInstanceSetNextFrameMask")
        if hasattr(lib, "XRSLAMAmdRenderTrackingView"):
            names["get_features"] = ("XRSLAMAmdGetFeatures", "XRSLAMAmdInstanceGetFeatures")
            names["set_feature_history"] = ("XRSLAMAmdSetFeatureHistory", "XRSLAMAmdInstanceSetFeatureHistory")
            names["render_tracking_view"] = ("XRSLAMAmdRenderTrackingView", "XRSLAMAmdInstanceRenderTrackingView")
        for attr, (glob, inst) in names.items():
            setattr(self, attr, getattr(lib, glob) if handle is None else functools.partial(getattr(lib, inst), handle))


def turn_frames(frames, o):
    """Frames [n][h][w] or [n][h][w][bytes per pixel] turned by orientation o = quarter turns clockwise + 4 * mirrored left to right
    first (include/XRSLAM.h: XRSLAMAmdSetFrameOrientation): [n][w][h]... for odd quarter turns, contiguous."""
    o = int(o)
    if not 0 <= o <= 7:
        raise ValueError("orientation %d is not 0..7" % o)
    f = frames[:, :, ::-1] if o >> 2 else frames
    return np.ascontiguousarray(np.rot90(f, -(o & 3), axes=(1, 2)))


def inverse_orientation(o):
    """The orientation that undoes o: a mirrored one undoes itself, a plain turn is undone by the opposite turn"""
    return int(o) if int(o) >> 2 else (4 - int(o)) & 3


class Session:
    """One XRSLAM instance: the process singleton behind the reference's six symbols (XRSLAMManager.cpp:6-9), or --
    instance=True -- an XRSLAMAmdInstance of its own, so that several sessions can live in one process.
    channels 3 / 4: seq["frames"] (or device_frames) hold interleaved BGR / BGRA frames, [n][h][w][channels].
    pixel_format (see frame_format): the frames are rows of bytes in that layout, [n][h][row bytes] (or [n][h][w][bytes per pixel]),
    pushed through XRSLAMAmdPushImageFormat / XRSLAMAmdInstanceReplayFormat from host memory or from device_frames.
    geometry (see frame_geometry): the frames are larger than cam0.resolution and go through XRSLAMAmdPushImageScaled /
    XRSLAMAmdInstanceReplayScaled, in pixel_format (None: GRAY8).
    orientation (0..7): every host frame of seq is turned by the INVERSE orientation here, as a camera mounted that way would deliver it,
    and XRSLAMAmdSetFrameOrientation(orientation) has the library turn it back in its upload: the run sees the original images.
    (device_frames are taken as they are: the caller stages them already turned, e.g. with turn_frames / inverse_orientation.)"""

    def __init__(self, lib_path, seq, slam_yaml=SLAM_YAML, sensor_yaml=SENSOR_YAML, device_frames=None,
                 init_frames=60, instance=False, device_undistort=None, threading=0, group=None, channels=1, pixel_format=None,
                 geometry=None, orientation=0):
        self.lib = load(lib_path)
        self.orientation = int(orientation)
        if self.orientation and device_frames is None:
            seq = dict(seq, frames=turn_frames(np.asarray(seq["frames"]), inverse_orientation(self.orientation)))
        self.channels = int(channels)
        self.pixel_format = None if pixel_format is None else frame_format(pixel_format)
        self.geometry = None if geometry is None else frame_geometry(geometry)
        self.seq = seq
        cfg = C.c_void_p()
        if instance:
            handle = C.c_void_p()
            ok = self.lib.XRSLAMAmdInstanceCreate(slam_yaml.encode(), sensor_yaml.encode(), C.byref(handle), C.byref(cfg))
            if ok != 1:
                raise RuntimeError("XRSLAMAmdInstanceCreate failed: %s" % self.lib.XRSLAMAmdLastError().decode())
            self.api = _Api(self.lib, handle)
            self._handle = handle
            if group is not None and self.lib.XRSLAMAmdInstanceJoinGroup(handle, group.handle) != 1:
                raise RuntimeError("XRSLAMAmdInstanceJoinGroup failed: %s" % self.api.last_error().decode())
        else:
            ok = self.lib.XRSLAMCreate(slam_yaml.encode(), sensor_yaml.encode(), b"", b"xrslam_amd", C.byref(cfg))
            if ok != 1:
                raise RuntimeError("XRSLAMCreate failed: %s" % self.lib.XRSLAMAmdLastError().decode())
            self.api = _Api(self.lib)
        if self.orientation:
            self.set_frame_orientation(self.orientation)
        if threading:   # 1 = backend of frame t beside the feature tracker of frame t+1 (XRSLAMAmdSetThreading)
            self.api.set_threading(int(threading))
        if device_undistort:   # frames are pushed as the camera recorded them and rectified on the GPU
            self.api.set_device_undistort(device_undistort.encode())
        st = seq["states"]
        for i in range(min(init_frames, len(st))):
            s = np.ascontiguousarray(st[i])
            q, p, v, bg, ba = [np.ascontiguousarray(s[a:b]) for a, b in ((0, 4), (4, 7), (7, 10), (10, 13), (13, 16))]
            self.api.set_initial_state(float(seq["cam_t"][i]), q.ctypes.data, p.ctypes.data, v.ctypes.data,
                                       bg.ctypes.data, ba.ctypes.data)
        self.device_frames = device_frames   # (base pointer, bytes per frame, stride) when frames live in HBM
        self.imu_k = 0
        self.frame_k = 0
        self.poses = []

    def _imu_structs(self):
        """The sensor structs of the whole sequence, built once (the player reads them from a file the same way);
        pushing a sample is then a single foreign call."""
        imu = self.seq["imu"]
        n = len(imu)
        gy, ac = (XRSLAMVec3 * n)(), (XRSLAMVec3 * n)()
        for k in range(n):
            r = imu[k]
            gy[k].data[0], gy[k].data[1], gy[k].data[2], gy[k].timestamp = r[1], r[2], r[3], r[0]
            ac[k].data[0], ac[k].data[1], ac[k].data[2], ac[k].timestamp = r[4], r[5], r[6], r[0]
        self._gy, self._ac = gy, ac
        self._imu_t = [float(v) for v in imu[:, 0]]

    def _push_imu_until(self, t_limit):
        if not hasattr(self, "_gy"):
            self._imu_structs()
        push, gy, ac, ts, n = self.api.push, self._gy, self._ac, self._imu_t, len(self._imu_t)
        k = self.imu_k
        lim = t_limit + 1e-9
        while k < n and ts[k] <= lim:
            push(XRSLAM_SENSOR_GYROSCOPE, C.byref(gy[k]))
            push(XRSLAM_SENSOR_ACCELERATION, C.byref(ac[k]))
            k += 1
        self.imu_k = k

    def _route(self):
        """How this session's frames reach the library, from what it holds now (channels / pixel_format / geometry may be set between
        steps): (push(ptr, stride, on_dev, t), name of the replay entry point, the arguments it takes between stride and on_device)."""
        api, ch = self.api, self.channels
        fmt = None if self.pixel_format is None else C.byref(self.pixel_format)
        if self.geometry is not None:
            geo = C.byref(self.geometry)
            return (lambda p, s, d, t: api.push_image_scaled(p, s, fmt, geo, d, t)), "XRSLAMAmdInstanceReplayScaled", (fmt, geo)
        if fmt is not None:
            return (lambda p, s, d, t: api.push_image_format(p, s, fmt, d, t)), "XRSLAMAmdInstanceReplayFormat", (fmt,)

        def push(p, s, d, t):
            if not d:
                api.push(XRSLAM_SENSOR_CAMERA, C.byref(XRSLAMImage(p.value, t, s, 0, ch, None)))
            elif ch == 1:
                api.push_image_device(p, s, t)
            else:
                api.push_image_device_color(p, s, ch, t)
        return (push, "XRSLAMAmdInstanceReplay", ()) if ch == 1 else (push, "XRSLAMAmdInstanceReplayColor", (ch,))

    def step(self):
        """Feeds everything up to and including the next camera frame; returns False at the end."""
        if self.frame_k >= len(self.seq["cam_t"]):
            return False
        t = float(self.seq["cam_t"][self.frame_k])
        self._push_imu_until(t)
        if self.device_frames is not None:
            base, fbytes, stride = self.device_frames
            ptr, on_dev = C.c_void_p(base + self.frame_k * fbytes), 1
        else:
            fr = self.seq["frames"][self.frame_k]
            ptr, stride, on_dev = C.c_void_p(fr.ctypes.data), fr.strides[0], 0
        self._route()[0](ptr, stride, on_dev, t)
        self.api.run()
        state = C.c_int(-1)
        self.api.get_result(XRSLAM_RESULT_STATE, C.byref(state))
        if state.value == 1:
            pose = XRSLAMPose()
            self.api.get_result(XRSLAM_RESULT_BODY_POSE, C.byref(pose))
            self.poses.append([pose.timestamp] + list(pose.translation) + list(pose.quaternion))
        self.frame_k += 1
        return True

    def step_n(self, n):
        """n camera frames through XRSLAMAmdInstanceReplay: the same call sequence as n x step(), issued natively (one
        foreign call, the interpreter lock released throughout) -- instance sessions only."""
        if not hasattr(self, "_rp"):
            imu = np.ascontiguousarray(self.seq["imu"], np.float64)
            cam_t = np.ascontiguousarray(self.seq["cam_t"], np.float64)
            frames = np.ascontiguousarray(self.seq["frames"])
            self._rp = (imu, cam_t, frames, C.c_int(self.imu_k), C.c_int(self.frame_k))
        imu, cam_t, frames, ic, fc = self._rp
        ic.value, fc.value = self.imu_k, self.frame_k
        out = np.zeros((max(n, 1), 8))
        if self.device_frames is not None:
            base, fbytes, stride = self.device_frames
            ptr, on_dev = C.c_void_p(base), 1
        else:
            ptr, fbytes, stride, on_dev = C.c_void_p(frames.ctypes.data), frames.strides[0], frames.strides[1], 0
        _, replay, extra = self._route()
        k = getattr(self.lib, replay)(self._handle, imu.ctypes.data, len(imu), cam_t.ctypes.data, len(cam_t), ptr, fbytes, stride, *extra,
                                      on_dev, C.byref(ic), C.byref(fc), int(n), out.ctypes.data)
        if k < 0:
            raise RuntimeError("XRSLAMAmdInstanceReplay: bad arguments")
        self.imu_k, self.frame_k = ic.value, fc.value
        for r in out[:k]:
            self.poses.append([r[0]] + list(r[1:4]) + list(r[4:8]))
        return k

    def set_frame_orientation(self, o):
        """XRSLAMAmdSetFrameOrientation: the frames pushed from now on are turned like that (the caller supplies them so)"""
        if self.api.set_frame_orientation(int(o)) != 1:
            raise RuntimeError("XRSLAMAmdSetFrameOrientation: %s" % self.error())

    def flush(self):
        """Pushes the IMU samples after the last frame so the last queued frame is processed
        (processing is triggered by the first IMU sample later than the frame, detail.cpp:130-142)."""
        self._push_imu_until(1e300)

    def sync(self):
        """Pipelined mode: waits for the backend job in flight (no-op otherwise)."""
        self.api.sync()

    def times(self):
        t = XRSLAMAmdTimes()
        self.api.get_times(C.byref(t))
        return t

    def set_profiling(self, on):
        self.api.set_profiling(1 if on else 0)

    def klt_stats(self, reset=False):
        from xrslam_amd.klt import KltStats
        st = KltStats()
        self.api.get_klt_stats(C.byref(st), 1 if reset else 0)
        return st

    def ba_stats(self, reset=False):
        st = BaStats()
        self.api.get_ba_stats(C.byref(st), 1 if reset else 0)
        return st

    @staticmethod
    def _mask_args(mask, on_device, stride):
        from xrslam_amd.abi import mask_args
        h, w = (0, 0) if mask is None or on_device else mask.shape
        return mask_args(mask, w, h, on_device, stride)

    def set_mask(self, mask, on_device=False, stride=None):
        """XRSLAMAmdSetMask: the static mask, a uint8 array [H][W] at the working resolution (or a device pointer with its stride);
        None clears it.  -> True, or False with the reason in last_error()."""
        ptr, stride = self._mask_args(mask, on_device, stride)
        return self.api.set_mask(ptr, stride, 1 if on_device else 0) == 1

    def set_next_frame_mask(self, mask, on_device=False, stride=None):
        """XRSLAMAmdSetNextFrameMask: the mask of the next camera frame pushed (consumed by it)."""
        ptr, stride = self._mask_args(mask, on_device, stride)
        return self.api.set_next_frame_mask(ptr, stride, 1 if on_device else 0) == 1

    def set_covariance(self, on):
        """XRSLAMAmdSetCovariance: every window solve is followed by the covariance of its newest keyframe"""
        self.api.set_covariance(1 if on else 0)

    def covariance(self):
        """-> (available, XRSLAMAmdCovariance): timestamp, state [15][15], pose_ros [6][6], status, rcond_estimate"""
        out = XRSLAMAmdCovariance()
        ok = self.api.get_covariance(C.byref(out))
        return ok == 1, out

    def landmark_variances(self):
        """-> (variances of the inverse depths, track ids) of the last window solve's free landmarks that are still valid"""
        n = self.api.get_landmark_variances(None, None, 0)
        var, ids = np.zeros(n), np.zeros(n, np.int64)
        if n:
            assert self.api.get_landmark_variances(var.ctypes.data, ids.ctypes.data, n) == n
        return var, ids

    def set_feature_history(self, frames):
        """Trail history of the feature snapshot, 0 .. 8 frames (XRSLAMAmdSetFeatureHistory)"""
        self.api.set_feature_history(int(frames))

    def features(self):
        """-> (timestamp, structured array FEATURE_DTYPE of all key points of the newest tracked frame), (None, empty) before it"""
        t = C.c_double(0)
        n = self.api.get_features(None, 0, C.byref(t))
        out = np.zeros(n, FEATURE_DTYPE)
        if n == 0:
            return None, out
        assert self.api.get_features(out.ctypes.data, n, C.byref(t)) == n
        return t.value, out

    def render_view(self, channels=3, color_mode=0, draw_new=0, trail=0, stride=None, out_dev=None):
        """XRSLAMAmdRenderTrackingView -> uint8 [h][w][channels], or None when the library answers 0 (see error()); with out_dev (a
        device pointer of rows `stride` bytes apart) the view stays in HBM and True is returned."""
        h, w = self.seq["frames"].shape[1:3]
        opt = XRSLAMAmdViewOptions(int(color_mode), int(draw_new), int(trail))
        stride = w * channels if stride is None else int(stride)
        if out_dev is not None:
            return True if self.api.render_tracking_view(C.c_void_p(int(out_dev)), stride, channels, 1, C.byref(opt)) == 1 else None
        buf = np.zeros(h * stride, np.uint8)
        if self.api.render_tracking_view(buf.ctypes.data, stride, channels, 0, C.byref(opt)) != 1:
            return None
        return np.lib.stride_tricks.as_strided(buf, shape=(h, w, channels), strides=(stride, channels, 1))

    def init_report(self):
        r = XRSLAMAmdInitReport()
        self.api.get_init_report(C.byref(r))
        return r

    def error(self):
        return self.api.last_error().decode()

    def close(self):
        self.api.destroy()


def ate_rmse(poses, seq):
    """ATE RMSE after SE(3) Umeyama alignment (what `evo_ape tum -a` computes, docs/en/tutorials/euroc_evaluation.md)."""
    if len(poses) < 3:
        return float("nan")
    P = np.array(poses)
    P = P[np.abs(P[:, 4:8]).sum(1) > 0]      # results before the first tracked frame are the all-zero pose (detail.cpp:165-168)
    if len(P) < 3:
        return float("nan")
    idx = np.searchsorted(seq["cam_t"], P[:, 0] - 1e-6)
    idx = np.clip(idx, 0, len(seq["cam_t"]) - 1)
    gt = seq["states"][idx, 4:7]
    est = P[:, 1:4]
    mu_e, mu_g = est.mean(0), gt.mean(0)
    H = (est - mu_e).T @ (gt - mu_g)
    U, S, Vt = np.linalg.svd(H)
    D = np.eye(3)
    if np.linalg.det(Vt.T @ U.T) < 0:
        D[2, 2] = -1
    R = Vt.T @ D @ U.T
    aligned = (R @ (est - mu_e).T).T + mu_g
    return float(np.sqrt(((aligned - gt) ** 2).sum(1).mean()))
