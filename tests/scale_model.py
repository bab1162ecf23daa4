"""Crop and area-scale of a camera frame in plain numpy: the yardstick of the frame-scaling tests.

A geometry is (src_width, src_height, crop_x, crop_y, cw, ch); the working plane is W x H with W <= cw, H <= ch and cw * ch <= 2^24.
g(i, j) is the gray value of source pixel (i, j) of the crop (tests/pixfmt_model.py: reduce, per source pixel, before averaging).
In units where a source pixel is W wide, working pixel X spans [X*cw, (X+1)*cw) and source column i covers [i*W, (i+1)*W); a_i is
the integer overlap of the two (the a_i of a working pixel sum to cw); b_j is the same vertically with ch and H.

    out(X, Y) = (sum_j b_j sum_i a_i g(i, j) + (cw*ch) // 2) // (cw*ch)

the exact area mean rounded half up: a crop for cw == W and ch == H, the k x k box mean for an integer ratio k.  Everything is an
integer here; 255 * cw * ch + cw * ch // 2 < 2^32 is what the implementations rely on.

`map_point` is the coordinate map that goes with it (pixel centres at integer coordinates), and `scale_intrinsics` what
XRSLAMAmdScaleIntrinsics computes from it."""
import numpy as np

from tests import pixfmt_model as pm

MAX_AREA = 1 << 24


def weights(n_out, n_in):
    """[n_out][n_in] int64: the overlap of output cell o = [o*n_in, (o+1)*n_in) with input cell i = [i*n_out, (i+1)*n_out)"""
    assert 1 <= n_out <= n_in
    o = np.arange(n_out, dtype=np.int64)[:, None]
    i = np.arange(n_in, dtype=np.int64)[None, :]
    wgt = np.maximum(0, np.minimum((i + 1) * n_out, (o + 1) * n_in) - np.maximum(i * n_out, o * n_in))
    assert (wgt.sum(1) == n_in).all() and (wgt.sum(0) == n_out).all()
    return wgt


def check(geo, W, H):
    sw, sh, x, y, cw, ch = geo
    assert x >= 0 and y >= 0 and cw >= 1 and ch >= 1 and x + cw <= sw and y + ch <= sh, geo
    assert W <= cw and H <= ch and cw * ch <= MAX_AREA, (geo, W, H)


def scale_gray(g, geo, W, H):
    """gray [..., src_height, src_width] uint8 -> [..., H, W] uint8"""
    check(geo, W, H)
    sw, sh, x, y, cw, ch = geo
    assert g.dtype == np.uint8 and g.shape[-2:] == (sh, sw), (g.shape, geo)
    crop = g[..., y:y + ch, x:x + cw].astype(np.float64)
    # the two matrix products run in float64 for speed and are exact: every operand is an integer and every partial sum is at most
    # 255 * cw * ch <= 255 * 2^24 < 2^53
    acc = (weights(H, ch).astype(np.float64) @ crop @ weights(W, cw).T.astype(np.float64)).astype(np.int64)
    area = cw * ch
    assert 0 <= acc.min(initial=0) and acc.max(initial=0) + area // 2 < 1 << 32
    return ((acc + area // 2) // area).astype(np.uint8)


def scale(px, geo, W, H, fmt=pm.GRAY8, bits=0, limited_range=0):
    """A frame [..., src_height, src_width, BYTES[fmt]] uint8 (rows may be strided) -> [..., H, W] uint8"""
    return scale_gray(pm.reduce(px, fmt, bits, limited_range), geo, W, H)


def replicate(g, kx, ky):
    """Every pixel of [..., h, w] repeated kx times horizontally and ky times vertically"""
    return np.repeat(np.repeat(g, ky, axis=-2), kx, axis=-1)


def map_point(u, v, geo, W, H):
    """A source pixel coordinate (pixel centres at integers) -> its working-image coordinate"""
    _, _, x, y, cw, ch = geo
    return (u + 0.5 - x) * W / cw - 0.5, (v + 0.5 - y) * H / ch - 0.5


def scale_intrinsics(K, geo, W, H):
    """(fx, fy, cx, cy) of the source camera -> those of the working image"""
    _, _, x, y, cw, ch = geo
    fx, fy, cx, cy = K
    return fx * W / cw, fy * H / ch, (cx + 0.5 - x) * W / cw - 0.5, (cy + 0.5 - y) * H / ch - 0.5
