"""ctypes mirror of plug point #1 (xrslam::Image, xrslam/include/xrslam/xrslam.h:137-161)
on top of the C ABI in include/xrslam_hip.h.  Method names and argument meaning
follow xrslam::extra::OpenCvImage (xrslam-extra/src/xrslam/extra/opencv_image.cpp)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .abi import FrameGeometry, mask_args, orientation


class KltStats(C.Structure):
    _fields_ = [("ms_preprocess", C.c_double), ("ms_track", C.c_double), ("ms_detect", C.c_double),
                ("n_preprocess", C.c_longlong), ("n_track", C.c_longlong), ("n_detect", C.c_longlong),
                ("lk_templates", C.c_longlong), ("lk_iterations", C.c_longlong), ("lk_points", C.c_longlong),
                ("detect_full_list", C.c_longlong)]


class LkParams(C.Structure):
    """xrhip_lk_params: cv::calcOpticalFlowPyrLK's winSize (square), maxLevel and criteria."""
    _fields_ = [("win", C.c_int), ("max_level", C.c_int), ("max_count", C.c_int), ("epsilon", C.c_double)]


LK_DEFAULTS = (21, 3, 30, 0.01)   # the reference's (opencv_image.cpp:96-99)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bind():
    L = _lib.lib()
    vp = C.c_void_p
    L.xrhip_klt_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.xrhip_klt_destroy.argtypes = [vp]
    L.xrhip_klt_destroy.restype = None
    L.xrhip_image_create.argtypes = [vp, C.POINTER(vp)]
    L.xrhip_image_upload.argtypes = [vp, vp, C.c_int]
    L.xrhip_image_upload_device.argtypes = [vp, vp, C.c_int]
    L.xrhip_image_destroy.argtypes = [vp]
    L.xrhip_image_destroy.restype = None
    L.xrhip_image_preprocess.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    L.xrhip_image_release.argtypes = [vp]
    L.xrhip_image_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, vp, C.POINTER(C.c_int)]
    L.xrhip_image_track.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_int]
    L.xrhip_image_lk.argtypes = [vp, vp, vp, vp, vp, C.c_int]
    L.xrhip_image_level_dims.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.xrhip_image_download_level.argtypes = [vp, C.c_int, vp, vp]
    L.xrhip_image_download_harris.argtypes = [vp, vp]
    L.xrhip_klt_set_profiling.argtypes = [vp, C.c_int]
    L.xrhip_klt_get_stats.argtypes = [vp, C.POINTER(KltStats), C.c_int]
    L.xrhip_klt_synchronize.argtypes = [vp]
    L.xrhip_klt_set_undistort_map.argtypes = [vp, vp]
    L.xrhip_image_upload_distorted.argtypes = [vp, vp, C.c_int, C.c_int]
    L.xrhip_image_upload_color.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.xrhip_image_upload_color_distorted.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.xrhip_image_upload_format.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.xrhip_image_upload_format_distorted.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.xrhip_image_upload_scaled.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FrameGeometry)]
    L.xrhip_image_upload_scaled_distorted.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FrameGeometry)]
    L.xrhip_debug_stream_span.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    L.xrhip_debug_get_raw.argtypes = [vp, vp]
    L.xrhip_debug_set_fused_pyramid.argtypes = [vp, C.c_int]
    L.xrhip_debug_get_level_padded.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.xrhip_image_render_view.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int]
    L.xrhip_debug_view_timing.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]
    L.xrhip_klt_set_lk_params.argtypes = [vp, C.POINTER(LkParams)]
    L.xrhip_klt_get_lk_params.argtypes = [vp, C.POINTER(LkParams)]
    L.xrhip_debug_force_general_lk.argtypes = [vp, C.c_int]
    L.xrhip_klt_set_mask.argtypes = [vp, vp, C.c_int, C.c_int]
    L.xrhip_image_set_mask.argtypes = [vp, vp, C.c_int, C.c_int]
    L.xrhip_debug_get_mask.argtypes = [vp, vp]
    if hasattr(L, "xrhip_klt_set_orientation"):   # (XRSLAM_HIP_LIB may name an earlier build's library: tools/orientation.py)
        L.xrhip_klt_set_orientation.argtypes = [vp, C.c_int]
        L.xrhip_klt_get_orientation.argtypes = [vp, C.POINTER(C.c_int)]
    return L


_L = None


def L():
    global _L
    if _L is None:
        _L = _bind()
    return _L




class KltContext:
    """One per sequence (owns the HIP stream and the CLAHE/GFTT state the reference keeps in statics)."""

    def __init__(self, width, height, max_points=200):
        self.w, self.h = int(width), int(height)
        h = C.c_void_p()
        check(L().xrhip_klt_create(self.w, self.h, int(max_points), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            L().xrhip_klt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def image(self, gray=None):
        return HipImage(self, gray)

    def set_profiling(self, on):
        check(L().xrhip_klt_set_profiling(self._h, 1 if on else 0))

    def stats(self, reset=False):
        s = KltStats()
        check(L().xrhip_klt_get_stats(self._h, C.byref(s), 1 if reset else 0))
        return s

    def synchronize(self):
        check(L().xrhip_klt_synchronize(self._h))

    def view_timing(self, enable=-1, reset=False):
        """HIP-event time of this context's renders (HipImage.render_view): -> (sum in ms, count); enable 1 / 0 switches it."""
        ms, n = C.c_double(0), C.c_longlong(0)
        check(L().xrhip_debug_view_timing(self._h, int(enable), C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def stream_span(self, phase):
        """HIP-event time of what the context issues between stream_span(0) and stream_span(1); the latter returns it in ms."""
        ms = C.c_double(0)
        check(L().xrhip_debug_stream_span(self._h, int(phase), C.byref(ms)))
        return ms.value

    def set_fused_pyramid(self, on):
        """Development / parity switch: preprocess() builds the pyramid in one launch (default) or in the five it replaces."""
        check(L().xrhip_debug_set_fused_pyramid(self._h, 1 if on else 0))

    def set_lk_params(self, win=None, max_level=None, max_count=None, epsilon=None):
        """Lucas-Kanade window (odd, 5..21), pyramid depth (0..5), iteration cap (1..100) and stop threshold (0..10) of this context;
        an argument left None takes the reference's value, no arguments at all restore 21 / 3 / 30 / 0.01.  Before the first image:
        the images' pyramid storage is sized by max_level.  HipImage.lk / track_keypoints need no new arguments."""
        if win is None and max_level is None and max_count is None and epsilon is None:
            check(L().xrhip_klt_set_lk_params(self._h, None))
            return
        d = LK_DEFAULTS
        p = LkParams(int(d[0] if win is None else win), int(d[1] if max_level is None else max_level),
                     int(d[2] if max_count is None else max_count), float(d[3] if epsilon is None else epsilon))
        check(L().xrhip_klt_set_lk_params(self._h, C.byref(p)))

    def get_lk_params(self):
        """-> (win, max_level, max_count, epsilon)"""
        p = LkParams()
        check(L().xrhip_klt_get_lk_params(self._h, C.byref(p)))
        return p.win, p.max_level, p.max_count, p.epsilon

    def force_general_lk(self, on):
        """Parity / measurement switch: the kernels with runtime parameters also at the reference's values."""
        check(L().xrhip_debug_force_general_lk(self._h, 1 if on else 0))

    def set_mask(self, mask, on_device=False, stride=None):
        """The static mask of this context (include/xrslam_hip.h, "Masks"): nonzero bytes may be used, zero bytes are excluded from
        detection and drop tracked points that land on them.  None clears it."""
        ptr, stride = mask_args(mask, self.w, self.h, on_device, stride)
        check(L().xrhip_klt_set_mask(self._h, ptr, stride, 1 if on_device else 0))

    def set_orientation(self, o):
        """Frames arrive turned or mirrored (include/xrslam_hip.h, xrhip_klt_set_orientation): o = quarter turns clockwise + 4 * mirrored
        first, 0..7 or a name of xrslam_amd.abi.ORIENT_NAMES.  Sticky, from the next upload on: an unscaled frame is then [w][h] for odd
        quarter turns, and the upload turns it into the plane."""
        check(L().xrhip_klt_set_orientation(self._h, orientation(o)))

    def get_orientation(self):
        if not hasattr(L(), "xrhip_klt_get_orientation"):
            return 0
        o = C.c_int(0)
        check(L().xrhip_klt_get_orientation(self._h, C.byref(o)))
        return o.value

    def frame_size(self):
        """(width, height) of an unscaled frame as the uploads read it under the current orientation"""
        return (self.h, self.w) if self.get_orientation() & 1 else (self.w, self.h)

    def set_undistort_map(self, map2):
        """Packed 1/32-pixel inverse map [h][w][2] uint32 (include/xrslam_hip.h), or None to switch the device
        undistortion off."""
        if map2 is None:
            check(L().xrhip_klt_set_undistort_map(self._h, None))
            return
        map2 = np.ascontiguousarray(map2, dtype=np.uint32)
        assert map2.shape == (self.h, self.w, 2), map2.shape
        check(L().xrhip_klt_set_undistort_map(self._h, _p(map2)))


class HipImage:
    """xrslam::Image on the MI355X."""

    def __init__(self, ctx, gray=None):
        self.ctx = ctx
        h = C.c_void_p()
        check(L().xrhip_image_create(ctx._h, C.byref(h)))
        self._h = h
        self.t = 0.0
        if gray is not None:
            self.upload(gray)

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            L().xrhip_image_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def width(self):
        return self.ctx.w

    def height(self):
        return self.ctx.h

    def level_num(self):
        return 3

    def upload(self, gray):
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
        assert gray.shape == self.ctx.frame_size()[::-1], gray.shape
        check(L().xrhip_image_upload(self._h, _p(gray), gray.strides[0]))

    def upload_distorted(self, gray):
        """The frame as the camera recorded it: rectified on the device (KltContext.set_undistort_map)."""
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
        assert gray.shape == self.ctx.frame_size()[::-1], gray.shape
        check(L().xrhip_image_upload_distorted(self._h, _p(gray), gray.strides[0], 0))

    def upload_distorted_device(self, dev_ptr, stride):
        check(L().xrhip_image_upload_distorted(self._h, C.c_void_p(dev_ptr), int(stride), 1))

    def _frame_args(self, pixels, on_device, stride, rows=None, interleaved=False):
        """-> (pointer, row stride in bytes) of a frame of `rows` rows (default: the plane's).  on_device: `pixels` is a device pointer
        (int) to row 0 and `stride` its row stride.  Otherwise a uint8 array of the frame's bytes, [rows][row bytes] or [rows][w][bytes
        per pixel] (interleaved: the latter, as wide as the plane); rows may be padded, pixels not."""
        if on_device:
            return C.c_void_p(int(pixels)), int(stride)
        fw, fh = self.ctx.frame_size()
        assert pixels.dtype == np.uint8 and pixels.ndim in (2, 3) and pixels.shape[0] == (rows or fh), pixels.shape
        assert not interleaved or (pixels.ndim == 3 and pixels.shape[1] == fw), pixels.shape
        assert pixels.strides[-1] == 1 and (pixels.ndim == 2 or pixels.strides[1] == pixels.shape[2]), pixels.strides
        return _p(pixels), pixels.strides[0]

    def _upload(self, fn, pixels, on_device, stride, *more, **how):
        ptr, stride = self._frame_args(pixels, on_device, stride, **how)
        check(fn(self._h, ptr, stride, *more))

    def upload_color(self, pixels, on_device=False, stride=None, channels=None):
        """An interleaved BGR / BGRA frame, reduced to gray on its way in: a uint8 array [h][w][3 or 4] (rows may be strided),
        or -- on_device -- a device pointer with its row stride in bytes and its channel count."""
        self._upload(L().xrhip_image_upload_color, pixels, on_device, stride, int(channels) if on_device else pixels.shape[2],
                     1 if on_device else 0, interleaved=True)

    def upload_color_distorted(self, pixels, on_device=False, stride=None, channels=None):
        """upload_color for a frame as the camera recorded it: reduced to gray, then rectified (KltContext.set_undistort_map)."""
        self._upload(L().xrhip_image_upload_color_distorted, pixels, on_device, stride, int(channels) if on_device else pixels.shape[2],
                     1 if on_device else 0, interleaved=True)

    def upload_format(self, pixels, fmt, bits=0, limited_range=0, on_device=False, stride=None):
        """A frame in one of the XRHIP_PIXFMT_* layouts (fmt: xrslam_amd.abi.PIXFMT_*, the Bayer mosaics PIXFMT_BAYER_* included), reduced
        to gray on its way in: a uint8 array of the frame's bytes, [h][row bytes] or [h][w][bytes per pixel] (rows may be strided), or
        -- on_device -- a device pointer with its row stride in bytes.  The packed 10 / 12-bit formats (abi.PIXFMT_PACKED): [h][row
        bytes], abi.packed_row_bytes(fmt, w) or more a row; `bits` is not read."""
        self._upload(L().xrhip_image_upload_format, pixels, on_device, stride, int(fmt), int(bits), int(limited_range), 1 if on_device else 0)

    def upload_format_distorted(self, pixels, fmt, bits=0, limited_range=0, on_device=False, stride=None):
        """upload_format for a frame as the camera recorded it: reduced to gray, then rectified (KltContext.set_undistort_map)."""
        self._upload(L().xrhip_image_upload_format_distorted, pixels, on_device, stride, int(fmt), int(bits), int(limited_range),
                     1 if on_device else 0)

    def upload_scaled(self, pixels, geo, fmt=0, bits=0, limited_range=0, on_device=False, stride=None, _fn="xrhip_image_upload_scaled"):
        """A frame larger than the context's plane, in any XRHIP_PIXFMT_* layout: the crop of `geo` = (src_width, src_height, crop_x,
        crop_y, crop_width, crop_height) is area-averaged down to the plane on its way in.  `pixels`: a uint8 array of the source
        frame's bytes, [src_height][row bytes] or [src_height][src_width][bytes per pixel] (rows may be strided), or -- on_device -- a
        device pointer to row 0 of the source frame with its row stride in bytes."""
        g = geo if isinstance(geo, FrameGeometry) else FrameGeometry(*[int(v) for v in geo])
        self._upload(getattr(L(), _fn), pixels, on_device, stride, int(fmt), int(bits), int(limited_range), 1 if on_device else 0, C.byref(g),
                     rows=g.src_height)

    def upload_scaled_distorted(self, pixels, geo, fmt=0, bits=0, limited_range=0, on_device=False, stride=None):
        """upload_scaled for a frame as the camera recorded it: scaled, then rectified (KltContext.set_undistort_map)."""
        self.upload_scaled(pixels, geo, fmt, bits, limited_range, on_device, stride, _fn="xrhip_image_upload_scaled_distorted")

    def set_mask(self, mask, on_device=False, stride=None):
        """The per-frame mask of the frame this image holds (after its upload, before preprocess / detect / track use it); combined
        with the context's static mask by AND.  None clears it; the next upload drops it."""
        ptr, stride = mask_args(mask, self.ctx.w, self.ctx.h, on_device, stride)
        check(L().xrhip_image_set_mask(self._h, ptr, stride, 1 if on_device else 0))

    def mask(self):
        """The frame's effective mask, uint8 [h][w] of 0 / 1 (parity aid; an error if the image has none)."""
        out = np.empty((self.ctx.h, self.ctx.w), np.uint8)
        check(L().xrhip_debug_get_mask(self._h, _p(out)))
        return out

    def raw(self):
        """The 8-bit frame preprocess() will read (parity aid)."""
        out = np.empty((self.ctx.h, self.ctx.w), np.uint8)
        check(L().xrhip_debug_get_raw(self._h, _p(out)))
        return out

    def render_view(self, segments=(), markers=(), palette=(), channels=3, stride=None, out=None, on_device=False):
        """The tracking view (xrhip_image_render_view): segments [n][5] = x0, y0, x1, y1, palette index; markers [n][4] = x, y, palette
        index, r2; palette [n][3] BGR.  -> uint8 [h][w][channels] (a view of rows `stride` bytes apart); with on_device, `out` is a
        device pointer, `stride` its row pitch, and nothing is returned (KltContext.synchronize completes it)."""
        sg = np.ascontiguousarray(np.asarray(segments, np.int64).reshape(-1, 5)).astype(np.int32)
        mk = np.asarray(markers, np.int64).reshape(-1, 4)
        mk3 = np.empty((len(mk), 3), np.int32)
        mk3[:, :2] = mk[:, :2]
        mk3[:, 2] = ((mk[:, 2] & 255) | (mk[:, 3] << 8)).astype(np.uint32).view(np.int32)
        pal = np.ascontiguousarray(np.asarray(palette, np.uint8).reshape(-1, 3))
        w, h = self.ctx.w, self.ctx.h
        if stride is None:
            stride = w * channels
        buf = None
        if on_device:
            ptr = C.c_void_p(int(out))
        else:
            buf = np.full(h * max(int(stride), 1) + 8, 0xA5, np.uint8) if out is None else out
            ptr = _p(buf)
        check(L().xrhip_image_render_view(self._h, _p(sg) if len(sg) else None, len(sg), _p(mk3) if len(mk3) else None, len(mk3),
                                          _p(pal) if len(pal) else None, len(pal), ptr, int(stride), int(channels), 1 if on_device else 0))
        if on_device:
            return None
        return np.lib.stride_tricks.as_strided(buf, shape=(h, w, channels), strides=(int(stride), channels, 1))

    def upload_device(self, dev_ptr, stride):
        check(L().xrhip_image_upload_device(self._h, C.c_void_p(int(dev_ptr)), int(stride)))

    def preprocess(self, clip=6.0, tiles_x=8, tiles_y=8):
        check(L().xrhip_image_preprocess(self._h, float(clip), int(tiles_x), int(tiles_y)))

    def release_image_buffer(self):
        check(L().xrhip_image_release(self._h))

    def prefetch_detect(self):
        """Hint: detect_keypoints will follow; the Harris pass is queued behind the next tracking launch onto this image."""
        check(L().xrhip_image_prefetch_detect(self._h))

    def detect_keypoints(self, existing, max_points, min_dist):
        existing = np.ascontiguousarray(existing, dtype=np.float64).reshape(-1, 2)
        out = np.empty((max(int(max_points), 1), 2), np.float64)
        n = C.c_int(0)
        check(L().xrhip_image_detect(self._h, _p(existing), len(existing), int(max_points), float(min_dist), _p(out),
                                     C.byref(n)))
        return np.concatenate([existing, out[:n.value]], axis=0)

    def track_keypoints(self, nxt, curr, guess=None):
        curr = np.ascontiguousarray(curr, dtype=np.float64).reshape(-1, 2)
        n = len(curr)
        if guess is None:
            nx = np.zeros_like(curr)
            has = 0
        else:
            nx = np.ascontiguousarray(guess, dtype=np.float64).reshape(-1, 2).copy()
            has = 1
        status = np.zeros(n, np.uint8)
        check(L().xrhip_image_track(self._h, nxt._h, _p(curr), _p(nx), has, _p(status), n))
        return nx, status

    def lk(self, nxt, prev_pts, next_pts):
        prev_pts = np.ascontiguousarray(prev_pts, dtype=np.float32).reshape(-1, 2)
        nx = np.ascontiguousarray(next_pts, dtype=np.float32).reshape(-1, 2).copy()
        status = np.zeros(len(prev_pts), np.uint8)
        check(L().xrhip_image_lk(self._h, nxt._h, _p(prev_pts), _p(nx), _p(status), len(prev_pts)))
        return nx, status

    def level(self, l):
        w = C.c_int()
        h = C.c_int()
        check(L().xrhip_image_level_dims(self._h, l, C.byref(w), C.byref(h)))
        img = np.empty((h.value, w.value), np.uint8)
        der = np.empty((h.value, w.value, 2), np.int16)
        check(L().xrhip_image_download_level(self._h, l, _p(img), _p(der)))
        return img, der

    def level_padded(self, l):
        """Level l's image plane with its 21-pixel reflect-101 border (what the LK windows read near the edges)."""
        rows, cols = C.c_int(), C.c_int()
        check(L().xrhip_debug_get_level_padded(self._h, l, None, C.byref(rows), C.byref(cols)))
        out = np.empty((rows.value, cols.value), np.uint8)
        check(L().xrhip_debug_get_level_padded(self._h, l, _p(out), C.byref(rows), C.byref(cols)))
        return out

    def harris(self):
        out = np.empty((self.ctx.h, self.ctx.w), np.float32)
        check(L().xrhip_image_download_harris(self._h, _p(out)))
        return out
