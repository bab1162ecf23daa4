"""OpenCvImage::track_keypoints with the Lucas-Kanade parameters as ARGUMENTS, restated in numpy from two OracleImage.lk calls
(oracle/klt_oracle.c: orc_lk takes window, depth, iteration cap and epsilon; orc_track_keypoints fixes them at 21 / 3 / 30 / 0.01)
and the three host-visible gates of orc_track_keypoints: the 20-pixel border, displacement <= rows / 4 (integer division, as in C),
forward-backward <= 0.5 with the backward status.  tests/test_lk_params_model.py pins it against orc_track_keypoints at the
reference's values; tests/test_lk_params_gpu.py uses it as the reference for xrhip_image_track at other values."""
import numpy as np

from oracle import klt_oracle as ko

_classes = {}


def oracle_class(max_level):
    """OracleImage whose pyramid has max_level + 1 levels (orc_pyr_create builds up to 8)."""
    if max_level not in _classes:
        _classes[max_level] = type("OracleImageL%d" % max_level, (ko.OracleImage,), {"MAX_LEVEL": int(max_level)})
    return _classes[max_level]


def oracle_image(gray, max_level, clahe=(6.0, 8, 8)):
    O = oracle_class(max_level)(gray)
    O.preprocess(*clahe)
    return O


def track_keypoints(OA, OB, curr, guess=None, win=21, max_level=3, max_count=30, eps=0.01):
    """-> (next [n][2] float64, status [n] uint8).  next holds the guess (zeros without one) where status is 0, as
    OracleImage.track_keypoints and HipImage.track_keypoints return it."""
    curr = np.ascontiguousarray(curr, dtype=np.float64).reshape(-1, 2)
    n = len(curr)
    out = np.zeros_like(curr) if guess is None else np.ascontiguousarray(guess, dtype=np.float64).reshape(-1, 2).copy()
    if n == 0:
        return out, np.zeros(0, np.uint8)
    cp = curr.astype(np.float32)
    start = cp.copy() if guess is None else out.astype(np.float32)
    cols, rows = OA.w, OA.h
    nxt, status, _ = OA.lk(OB, cp, start, max_level=max_level, max_count=max_count, eps=eps, win=win)
    status = status.copy()
    x, y = nxt[:, 0], nxt[:, 1]
    status[(x < np.float32(20)) | (x >= np.float32(cols - 20)) | (y < np.float32(20)) | (y >= np.float32(rows - 20))] = 0
    d = nxt - cp                                                  # float32
    nrm = np.sqrt(d[:, 0].astype(np.float64) ** 2 + d[:, 1].astype(np.float64) ** 2)
    status[nrm > rows // 4] = 0
    back, st2, _ = OB.lk(OA, nxt, cp.copy(), max_level=max_level, max_count=max_count, eps=eps, win=win)
    d = cp - back
    nrm = np.sqrt(d[:, 0].astype(np.float64) ** 2 + d[:, 1].astype(np.float64) ** 2)
    status[(st2 == 0) | (nrm > 0.5)] = 0
    ok = status != 0
    out[ok] = nxt[ok].astype(np.float64)
    return out, status
