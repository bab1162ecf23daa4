"""ctypes mirrors of the plain-C structs declared in include/xrslam_hip.h (layout only, no logic)."""
import copy
import ctypes as C

import numpy as np

STATE_DIM = 16
ES_DIM = 15
IMU_DIM = 281
FIX_POSE = 1
FIX_MOTION = 2

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_bp = C.POINTER(C.c_uint8)


class BaProblem(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int), ("frame_state", _dp), ("frame_fix", _bp),
        ("cam_q_bc", C.c_double * 4), ("cam_p_bc", C.c_double * 3),
        ("imu_q_bi", C.c_double * 4), ("imu_p_bi", C.c_double * 3),
        ("sqrt_inv_cov", C.c_double * 2),
        ("n_landmarks", C.c_int), ("inv_depth", _dp), ("landmark_fix", _bp),
        ("n_obs", C.c_int), ("obs_tgt", _ip), ("obs_ref", _ip), ("obs_lm", _ip),
        ("obs_z_tgt", _dp), ("obs_z_ref", _dp),
        ("n_rot", C.c_int), ("rot_tgt", _ip), ("rot_ref", _ip), ("rot_z_tgt", _dp), ("rot_z_ref", _dp),
        ("n_imu", C.c_int), ("imu_i", _ip), ("imu_j", _ip), ("imu_data", _dp),
        ("prior_n", C.c_int), ("prior_frames", _ip), ("prior_sqrt_info", _dp), ("prior_infovec", _dp),
        ("prior_lin", _dp),
        ("max_iterations", C.c_int),
    ]


class BaSummary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("successful_steps", C.c_int), ("termination", C.c_int),
                ("usable", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("ms_solve", C.c_double)]


class CovRequest(C.Structure):   # xrhip_cov_request
    _fields_ = [("n_sel", C.c_int), ("sel_frames", _ip), ("out_blocks", _dp), ("out_inv_depth_var", _dp), ("status", _ip),
                ("rcond_estimate", _dp)]


class MargProblem(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int), ("victim", C.c_int), ("frame_state", _dp),
        ("cam_q_bc", C.c_double * 4), ("cam_p_bc", C.c_double * 3),
        ("imu_q_bi", C.c_double * 4), ("imu_p_bi", C.c_double * 3),
        ("sqrt_inv_cov", C.c_double * 2),
        ("prior_n", C.c_int), ("prior_frames", _ip), ("prior_sqrt_info", _dp), ("prior_infovec", _dp),
        ("prior_lin", _dp),
        ("n_imu", C.c_int), ("imu_i", _ip), ("imu_j", _ip), ("imu_data", _dp),
        ("n_landmarks", C.c_int), ("inv_depth", _dp),
        ("n_obs", C.c_int), ("obs_tgt", _ip), ("obs_ref", _ip), ("obs_lm", _ip),
        ("obs_z_tgt", _dp), ("obs_z_ref", _dp),
    ]


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _dpp(a):
    return a.ctypes.data_as(_dp)


def _ipp(a):
    return a.ctypes.data_as(_ip)


class _Factors:
    """shared unpacking of the factor dictionaries"""

    def _set_obs(self, o):
        o = o or {}
        self.obs_tgt = _arr(o.get("tgt", []), np.int32)
        self.obs_ref = _arr(o.get("ref", []), np.int32)
        self.obs_lm = _arr(o.get("lm", []), np.int32)
        self.obs_z_tgt = _arr(o.get("z_tgt", np.zeros((0, 3))), np.float64).reshape(-1, 3)
        self.obs_z_ref = _arr(o.get("z_ref", np.zeros((0, 3))), np.float64).reshape(-1, 3)

    def _set_imu(self, m):
        m = m or {}
        self.imu_i = _arr(m.get("i", []), np.int32)
        self.imu_j = _arr(m.get("j", []), np.int32)
        self.imu_data = _arr(m.get("data", np.zeros((0, IMU_DIM))), np.float64).reshape(-1, IMU_DIM)

    def _set_prior(self, p):
        p = p or {}
        self.prior_frames = _arr(p.get("frames", []), np.int32)
        n = ES_DIM * len(self.prior_frames)
        self.prior_sqrt_info = _arr(p.get("sqrt_info", np.zeros((n, n))), np.float64).reshape(n, n)
        self.prior_infovec = _arr(p.get("infovec", np.zeros(n)), np.float64)
        self.prior_lin = _arr(p.get("lin", np.zeros((len(self.prior_frames), STATE_DIM))), np.float64)

    def _fill_common(self, s):
        s.cam_q_bc[:] = list(self.cam_ext[:4])
        s.cam_p_bc[:] = list(self.cam_ext[4:7])
        s.imu_q_bi[:] = list(self.imu_ext[:4])
        s.imu_p_bi[:] = list(self.imu_ext[4:7])
        s.sqrt_inv_cov[:] = list(self.sqrt_inv_cov[:2])
        s.n_obs = len(self.obs_tgt)
        s.obs_tgt, s.obs_ref, s.obs_lm = _ipp(self.obs_tgt), _ipp(self.obs_ref), _ipp(self.obs_lm)
        s.obs_z_tgt, s.obs_z_ref = _dpp(self.obs_z_tgt), _dpp(self.obs_z_ref)
        s.n_imu = len(self.imu_i)
        s.imu_i, s.imu_j, s.imu_data = _ipp(self.imu_i), _ipp(self.imu_j), _dpp(self.imu_data)
        s.prior_n = len(self.prior_frames)
        s.prior_frames = _ipp(self.prior_frames)
        s.prior_sqrt_info, s.prior_infovec = _dpp(self.prior_sqrt_info), _dpp(self.prior_infovec)
        s.prior_lin = _dpp(self.prior_lin)


class BaProblemData(_Factors):
    """numpy-side owner of a BA problem; .struct() returns the C view (arrays stay alive with self)."""

    def __init__(self, frame_state, frame_fix, cam_ext, imu_ext, sqrt_inv_cov, inv_depth, landmark_fix=None,
                 obs=None, rot=None, imu=None, prior=None, max_iterations=30):
        self.frame_state = _arr(frame_state, np.float64).reshape(-1, STATE_DIM).copy()
        self.frame_fix = _arr(frame_fix, np.uint8).copy()
        self.cam_ext = _arr(cam_ext, np.float64)
        self.imu_ext = _arr(imu_ext, np.float64)
        self.sqrt_inv_cov = _arr(sqrt_inv_cov, np.float64)
        self.inv_depth = _arr(inv_depth, np.float64).copy()
        nl = len(self.inv_depth)
        self.landmark_fix = _arr(landmark_fix if landmark_fix is not None else np.zeros(nl), np.uint8).copy()
        self._set_obs(obs)
        r = rot or {}
        self.rot_tgt = _arr(r.get("tgt", []), np.int32)
        self.rot_ref = _arr(r.get("ref", []), np.int32)
        self.rot_z_tgt = _arr(r.get("z_tgt", np.zeros((0, 3))), np.float64).reshape(-1, 3)
        self.rot_z_ref = _arr(r.get("z_ref", np.zeros((0, 3))), np.float64).reshape(-1, 3)
        self._set_imu(imu)
        self._set_prior(prior)
        self.max_iterations = int(max_iterations)

    def copy(self):
        return copy.deepcopy(self)

    def struct(self):
        s = BaProblem()
        s.n_frames = len(self.frame_state)
        s.frame_state = _dpp(self.frame_state)
        s.frame_fix = self.frame_fix.ctypes.data_as(_bp)
        s.n_landmarks = len(self.inv_depth)
        s.inv_depth = _dpp(self.inv_depth)
        s.landmark_fix = self.landmark_fix.ctypes.data_as(_bp)
        self._fill_common(s)
        s.n_rot = len(self.rot_tgt)
        s.rot_tgt, s.rot_ref = _ipp(self.rot_tgt), _ipp(self.rot_ref)
        s.rot_z_tgt, s.rot_z_ref = _dpp(self.rot_z_tgt), _dpp(self.rot_z_ref)
        s.max_iterations = self.max_iterations
        return s


class MargProblemData(_Factors):
    def __init__(self, frame_state, victim, cam_ext, imu_ext, sqrt_inv_cov, prior, imu, inv_depth, obs):
        self.frame_state = _arr(frame_state, np.float64).reshape(-1, STATE_DIM).copy()
        self.victim = int(victim)
        self.cam_ext = _arr(cam_ext, np.float64)
        self.imu_ext = _arr(imu_ext, np.float64)
        self.sqrt_inv_cov = _arr(sqrt_inv_cov, np.float64)
        self._set_prior(prior)
        self._set_imu(imu)
        self.inv_depth = _arr(inv_depth, np.float64).copy()
        self._set_obs(obs)

    def struct(self):
        s = MargProblem()
        s.n_frames = len(self.frame_state)
        s.victim = self.victim
        s.frame_state = _dpp(self.frame_state)
        self._fill_common(s)
        s.n_landmarks = len(self.inv_depth)
        s.inv_depth = _dpp(self.inv_depth)
        return s
# XRHIP_PIXFMT_* (include/xrslam_hip.h) = XRSLAMAmdPixelFormat (include/XRSLAM.h)
PIXFMT_GRAY8, PIXFMT_BGR8, PIXFMT_BGRA8, PIXFMT_RGB8, PIXFMT_RGBA8, PIXFMT_GRAY16, PIXFMT_YUYV, PIXFMT_UYVY, PIXFMT_NV12, \
    PIXFMT_I420, PIXFMT_P010 = range(11)
PIXFMT_BYTES = {PIXFMT_GRAY8: 1, PIXFMT_BGR8: 3, PIXFMT_BGRA8: 4, PIXFMT_RGB8: 3, PIXFMT_RGBA8: 4, PIXFMT_GRAY16: 2, PIXFMT_YUYV: 2,
                PIXFMT_UYVY: 2, PIXFMT_NV12: 1, PIXFMT_I420: 1, PIXFMT_P010: 2}   # bytes per pixel read (NV12 / I420 / P010: the luma plane's)
# Bayer raw mosaics, named by the top-left 2 x 2 tile read row by row (11..15 are not formats); *8: one byte per sample, *16: two
PIXFMT_BAYER_RGGB8, PIXFMT_BAYER_GRBG8, PIXFMT_BAYER_GBRG8, PIXFMT_BAYER_BGGR8, PIXFMT_BAYER_RGGB16, PIXFMT_BAYER_GRBG16, \
    PIXFMT_BAYER_GBRG16, PIXFMT_BAYER_BGGR16 = range(16, 24)
PIXFMT_BAYER_BYTES = {f: 1 if f < PIXFMT_BAYER_RGGB16 else 2 for f in range(16, 24)}
# Packed 10 / 12-bit samples (24..31, 36..39 and 56.. are not formats).  Packings in format-number order: CSI-2 RAW10 / RAW12 groups,
# then the PFNC lsb-packed bit streams; GRAY = 32 + packing, BAYER = 40 + 4 * packing + pattern (the patterns in the order above)
PACKINGS = (("mipi", 10), ("mipi", 12), ("lsb", 10), ("lsb", 12))
PIXFMT_GRAY10_MIPI, PIXFMT_GRAY12_MIPI, PIXFMT_GRAY10P, PIXFMT_GRAY12P = range(32, 36)
PIXFMT_BAYER_RGGB10_MIPI, PIXFMT_BAYER_GRBG10_MIPI, PIXFMT_BAYER_GBRG10_MIPI, PIXFMT_BAYER_BGGR10_MIPI, \
    PIXFMT_BAYER_RGGB12_MIPI, PIXFMT_BAYER_GRBG12_MIPI, PIXFMT_BAYER_GBRG12_MIPI, PIXFMT_BAYER_BGGR12_MIPI, \
    PIXFMT_BAYER_RGGB10P, PIXFMT_BAYER_GRBG10P, PIXFMT_BAYER_GBRG10P, PIXFMT_BAYER_BGGR10P, \
    PIXFMT_BAYER_RGGB12P, PIXFMT_BAYER_GRBG12P, PIXFMT_BAYER_GBRG12P, PIXFMT_BAYER_BGGR12P = range(40, 56)
# format -> (packing, bits, Bayer phase (px, py) of RGGB or None for the mono forms)
PIXFMT_PACKED = {32 + p: PACKINGS[p] + (None,) for p in range(4)}
PIXFMT_PACKED.update({40 + 4 * p + k: PACKINGS[p] + ((k & 1, k >> 1),) for p in range(4) for k in range(4)})


def packed_row_bytes(fmt, width):
    """bytes that hold a row of `width` pixels of the packed format `fmt`"""
    packing, bits, _ = PIXFMT_PACKED[fmt]
    if packing == "mipi":
        return (5 * ((width + 3) // 4)) if bits == 10 else (3 * ((width + 1) // 2))
    return (bits * width + 7) // 8


class FrameGeometry(C.Structure):
    """xrhip_frame_geometry = XRSLAMAmdFrameGeometry: the crop of a src_width x src_height frame that becomes the working image"""
    _fields_ = [("src_width", C.c_int), ("src_height", C.c_int), ("crop_x", C.c_int), ("crop_y", C.c_int), ("crop_width", C.c_int),
                ("crop_height", C.c_int)]


# Frame orientations (xrhip_klt_set_orientation = XRSLAMAmdSetFrameOrientation): o = r + 4 f -- mirrored left to right first if f, then r
# quarter turns clockwise
ORIENT_NONE, ORIENT_ROT90, ORIENT_ROT180, ORIENT_ROT270, ORIENT_FLIP, ORIENT_FLIP_ROT90, ORIENT_FLIP_ROT180, ORIENT_FLIP_ROT270 = range(8)
ORIENT_NAMES = {"none": 0, "rot90": 1, "rot180": 2, "rot270": 3, "flip": 4, "flip-rot90": 5, "flip-rot180": 6, "flip-rot270": 7,
                "transverse": 5, "flipv": 6, "transpose": 7}


def orientation(o):
    """An orientation given as 0..7 or by name (ORIENT_NAMES) -> 0..7"""
    if isinstance(o, str):
        if o not in ORIENT_NAMES and not (o.isdigit() and int(o) < 8):
            raise ValueError("orientation %r is not one of %s or 0..7" % (o, ", ".join(ORIENT_NAMES)))
        return ORIENT_NAMES[o] if o in ORIENT_NAMES else int(o)
    return int(o)


def mask_args(mask, w, h, on_device=False, stride=None):
    """-> (pointer, row stride in bytes) of a w x h byte mask for xrhip_klt_set_mask / xrhip_image_set_mask / XRSLAMAmdSetMask /
    XRSLAMAmdSetNextFrameMask: None (clears), a uint8 array [h][w] whose rows may be strided (the caller keeps it alive for the call), or
    -- on_device -- a device pointer (int) with its row stride.  `stride` overrides the array's own."""
    if mask is None:
        return None, 0
    if on_device:
        return C.c_void_p(int(mask)), int(stride)
    assert mask.dtype == np.uint8 and mask.shape == (h, w) and mask.strides[1] == 1, (mask.dtype, mask.shape, mask.strides)
    return C.c_void_p(mask.ctypes.data), mask.strides[0] if stride is None else int(stride)
