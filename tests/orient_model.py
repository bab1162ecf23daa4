"""Turned and mirrored camera frames in plain numpy: the yardstick of the orientation tests.

An orientation is o = r + 4*f, 0..7.  It acts on the gray crop c(i, j), 0 <= i < cw, 0 <= j < ch (after format reduction or
demosaicing and cropping, before scaling):

    f set: mirror left to right first   c'(i, j) = c(cw-1-i, j)          (else c' = c)
    then r quarter turns clockwise      r = 1: u(X, Y) = c'(Y, ch-1-X)         u is ch x cw
                                        r = 2: u(X, Y) = c'(cw-1-X, ch-1-Y)
                                        r = 3: u(X, Y) = c'(cw-1-Y, X)         u is ch x cw

The turned crop u is then area-scaled to the working plane (tests/scale_model.py).  Arrays are [row, column] = [j, i] / [Y, X].

`map_point` is the coordinate map that goes with it (pixel centres at integer coordinates), `orient_intrinsics` what
XRSLAMAmdOrientIntrinsics computes from it, `from_exif` the EXIF orientation tag's table."""
import numpy as np

EXIF = {1: 0, 6: 1, 3: 2, 8: 3, 2: 4, 7: 5, 4: 6, 5: 7}


def turned_size(cw, ch, o):
    return (ch, cw) if o & 1 else (cw, ch)


def orient(g, o):
    """[..., ch, cw] -> the turned [..., H, W], written from the formulas with index arithmetic"""
    assert 0 <= o <= 7
    ch, cw = g.shape[-2:]
    r, f = o & 3, o >> 2
    W, H = turned_size(cw, ch, o)
    Y, X = np.mgrid[0:H, 0:W]
    if r == 0:
        i, j = X, Y
    elif r == 1:
        i, j = Y, ch - 1 - X
    elif r == 2:
        i, j = cw - 1 - X, ch - 1 - Y
    else:
        i, j = cw - 1 - Y, X
    if f:
        i = cw - 1 - i
    return np.ascontiguousarray(g[..., j, i])


def orient_rot90(g, o):
    """The same with numpy's own mirror and quarter turn (np.rot90 turns anticlockwise for positive k)"""
    assert 0 <= o <= 7
    c = g[..., :, ::-1] if o >> 2 else g
    return np.ascontiguousarray(np.rot90(c, -(o & 3), axes=(-2, -1)))


def inverse(o):
    """The orientation that undoes o: a mirrored one undoes itself (M R^-r = R^r M), a turn is undone by the opposite turn"""
    assert 0 <= o <= 7
    return o if o >> 2 else (4 - o) & 3


def map_point(i, j, o, cw, ch):
    """Where pixel (i, j) of the cw x ch crop lies in the turned crop"""
    r = o & 3
    if o >> 2:
        i = cw - 1 - i
    if r == 0:
        return i, j
    if r == 1:
        return ch - 1 - j, i
    if r == 2:
        return cw - 1 - i, ch - 1 - j
    return j, cw - 1 - i


def source_geometry(geo, o, W, H):
    """(crop_x, crop_y, cw, ch) of a geometry; None: the whole frame, which is H x W in memory for odd r"""
    if geo is None:
        cw, ch = turned_size(W, H, o)
        return 0, 0, cw, ch
    return geo[2], geo[3], geo[4], geo[5]


def map_frame_point(u, v, geo, o, W, H):
    """A source pixel coordinate -> its working-image coordinate: crop, turn, scale"""
    x, y, cw, ch = source_geometry(geo, o, W, H)
    X, Y = map_point(u - x, v - y, o, cw, ch)
    tw, th = turned_size(cw, ch, o)
    return (X + 0.5) * W / tw - 0.5, (Y + 0.5) * H / th - 0.5


def orient_intrinsics(K, geo, o, W, H):
    """(fx, fy, cx, cy) of the source camera -> (those of the working image, R): R takes a ray of the source camera to the working
    camera's, a signed permutation of x and y (a reflection for mirrored orientations)"""
    x, y, cw, ch = source_geometry(geo, o, W, H)
    p0 = np.array(map_point(0, 0, o, cw, ch), dtype=np.float64)
    P = np.stack([np.array(map_point(1, 0, o, cw, ch)) - p0, np.array(map_point(0, 1, o, cw, ch)) - p0], axis=1)
    tw, th = turned_size(cw, ch, o)
    S = np.diag([W / tw, H / th])
    fx, fy, cx, cy = K
    F = S @ np.abs(P) @ np.array([fx, fy])
    c = S @ (P @ np.array([cx - x, cy - y]) + p0 + 0.5) - 0.5
    R = np.eye(3)
    R[:2, :2] = P
    return (F[0], F[1], c[0], c[1]), R


def from_exif(tag):
    return EXIF.get(tag, -1)
