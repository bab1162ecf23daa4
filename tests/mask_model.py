"""Detection and tracking under a mask, restated in numpy and plain loops (include/xrslam_hip.h, "Masks").

Independent of the library and of the oracle's code: the oracle (oracle/klt_oracle.c) has no mask argument, so this model is what the
masked device path is compared against, and tests/test_mask_model.py first shows that with an all-ones mask it IS the oracle's
detect_keypoints, key point for key point.

detect(resp, mask, existing, max_points, min_distance) is cv::goodFeaturesToTrack(image, ..., mask) as OpenCvImage::detect_keypoints
calls it, followed by that function's Poisson-disk filter and border rule:
  1. the maximum of the response over pixels whose mask byte is nonzero,
  2. threshold = (float)(max * 1e-3); responses not above it count as 0,
  3. a pixel survives the 3x3 non-maximum suppression if it is nonzero and equals the maximum of its 3x3 neighbourhood -- all eight
     neighbours, masked or not -- and only interior pixels are tested,
  4. ... and if its own mask byte is nonzero,
  5. visiting order: response descending, then linear index descending,
  6. greedy spacing: a corner is taken if no corner taken before lies closer than 20 pixels, until max_points are taken,
  7. the Poisson-disk filter of radius min_distance against the existing points (and the corners accepted before), with the
     reference filter's scan quirk, then the 20-pixel border rule."""
import math

import numpy as np

QUALITY = 1.0e-3
SPACING = 20.0   # the literal minDistance of the reference's GFTTDetector
BORDER = 20


def masked_max(resp, mask):
    """The largest response among visible pixels, or None when no pixel is visible."""
    vis = np.asarray(mask) != 0
    if not vis.any():
        return None
    return np.float32(resp[vis].max())


def threshold(resp, mask):
    m = masked_max(resp, mask)
    return None if m is None else np.float32(np.float64(m) * QUALITY)


def candidates(resp, mask):
    """-> (linear indices, responses) of the NMS survivors in visiting order."""
    resp = np.asarray(resp, np.float32)
    h, w = resp.shape
    thr = threshold(resp, mask)
    if thr is None:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    e = np.where(resp > thr, resp, np.float32(0)).astype(np.float32)
    dil = e[1:-1, 1:-1].copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            dil = np.maximum(dil, e[dy:dy + h - 2, dx:dx + w - 2])
    flag = np.zeros((h, w), bool)
    c = e[1:-1, 1:-1]
    flag[1:-1, 1:-1] = (c != 0) & (c == dil) & (np.asarray(mask)[1:-1, 1:-1] != 0)
    idx = np.flatnonzero(flag)
    v = e.reshape(-1)[idx]
    order = np.lexsort((-idx, -v.astype(np.float64)))
    return idx[order], v[order]


def spaced(idx, w, h, max_points, min_distance=SPACING):
    """The greedy minimum-distance pass of goodFeaturesToTrack over candidates in visiting order -> [(x, y)] ints."""
    cell = int(round(min_distance))
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    grid = {}
    out = []
    md2 = min_distance * min_distance
    for i in idx:
        y, x = divmod(int(i), w)
        xc, yc = x // cell, y // cell
        good = True
        for yy in range(max(yc - 1, 0), min(yc + 1, gh - 1) + 1):
            for xx in range(max(xc - 1, 0), min(xc + 1, gw - 1) + 1):
                for (px, py) in grid.get((xx, yy), ()):
                    if (x - px) * (x - px) + (y - py) * (y - py) < md2:
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid.setdefault((xc, yc), []).append((x, y))
            out.append((x, y))
            if max_points > 0 and len(out) == max_points:
                break
    return out


class PoissonDisk:
    """PoissonDiskFilter<2> of the reference: cells of radius / sqrt(2) that remember the LAST point put into them; a test scans the
    5 x 5 cells around the point's, skipping the first cell of the box and visiting one cell below its first column instead."""

    def __init__(self, radius):
        self.r2 = radius * radius
        self.grid = radius / math.sqrt(2.0)
        self.span = int(math.ceil(math.sqrt(2.0)))
        self.cells = {}

    def _cell(self, x, y):
        return int(math.floor(x / self.grid)), int(math.floor(y / self.grid))

    def preset(self, x, y):
        self.cells[self._cell(x, y)] = (x, y)

    def permits(self, x, y):
        ix, iy = self._cell(x, y)
        bx, by, ex, ey = ix - self.span, iy - self.span, ix + self.span, iy + self.span
        cx, cy = bx, by
        while cy <= ey:
            cx += 1
            if cx > ex:
                cx = bx
                cy += 1
            p = self.cells.get((cx, cy))
            if p is not None:
                dx, dy = x - p[0], y - p[1]
                if dx * dx + dy * dy < self.r2:
                    return False
        return True


def detect(resp, mask, existing, max_points, min_distance):
    """-> the NEW key points, float64 [n][2], in the order the reference appends them."""
    resp = np.asarray(resp, np.float32)
    h, w = resp.shape
    idx, _ = candidates(resp, mask)
    corners = spaced(idx, w, h, max_points)
    out = []
    if corners:
        f = PoissonDisk(float(min_distance))
        for x, y in np.asarray(existing, np.float64).reshape(-1, 2):
            f.preset(float(x), float(y))
        for x, y in corners:
            x, y = float(x), float(y)
            if not f.permits(x, y):
                continue
            f.preset(x, y)
            if x < BORDER or y < BORDER or x >= w - BORDER or y >= h - BORDER:
                continue
            out.append((x, y))
    return np.asarray(out, np.float64).reshape(-1, 2)


def track_gate(next_xy, status, mask):
    """The mask gate behind the reference's gates: a point with status != 0 at (x, y) is dropped when the mask is zero at
    (floor(x + 0.5), floor(y + 0.5)).  -> the gated status (positions of dropped points are not reported)."""
    st = np.array(status, np.uint8).copy()
    for i, (x, y) in enumerate(np.asarray(next_xy, np.float64).reshape(-1, 2)):
        if st[i] and mask[int(math.floor(y + 0.5)), int(math.floor(x + 0.5))] == 0:
            st[i] = 0
    return st


def on_zero_byte(xy, mask):
    """Which of the points have their nearest pixel on a zero byte (points outside the plane count as on one)."""
    h, w = mask.shape
    out = []
    for x, y in np.asarray(xy, np.float64).reshape(-1, 2):
        px, py = int(math.floor(x + 0.5)), int(math.floor(y + 0.5))
        out.append(not (0 <= px < w and 0 <= py < h) or mask[py, px] == 0)
    return np.asarray(out, bool)
