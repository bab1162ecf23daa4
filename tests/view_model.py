"""The tracking view (include/xrslam_hip.h: xrhip_image_render_view) restated in plain Python loops: the model the device renderer is
held to, bit for bit.  It shares no code with the library.

    canvas    gray replicated to B = G = R (channels 4: fourth byte 255)
    segment   (x0, y0, x1, y1, palette index): n = max(|dx|, |dy|); pixel k = 0..n is x0 + floor((2 k dx + n) / (2 n)), y likewise
              (Python's // IS floor division); n = 0 is the pixel (x0, y0)
    marker    (x, y, palette index, r2): every pixel with dx^2 + dy^2 <= r2
    clipping  pixels outside the image are dropped
    priority  any marker above any segment above the canvas; within a list the later entry wins -- so painting the segments in list
              order and then the markers in list order, each pixel simply overwritten, is the definition itself
"""
import numpy as np


def segment_pixels(x0, y0, x1, y1):
    """The n + 1 pixels of a segment, unclipped, in order k = 0..n."""
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(x0, y0)]
    return [(x0 + (2 * k * dx + n) // (2 * n), y0 + (2 * k * dy + n) // (2 * n)) for k in range(n + 1)]


def marker_pixels(x, y, r2):
    """The pixels of a disc, unclipped."""
    r = 0
    while (r + 1) * (r + 1) <= r2:
        r += 1
    return [(x + dx, y + dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r2]


def _clipped_segment(x0, y0, x1, y1, w, h):
    """segment_pixels restricted to the image without walking the part of a long segment that lies outside"""
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(x0, y0)] if 0 <= x0 < w and 0 <= y0 < h else []
    out = []
    for k in range(n + 1):
        x = x0 + (2 * k * dx + n) // (2 * n)
        if x < 0 or x >= w:
            continue
        y = y0 + (2 * k * dy + n) // (2 * n)
        if 0 <= y < h:
            out.append((x, y))
    return out


def render(gray, segments=(), markers=(), palette=(), channels=3):
    """gray uint8 [h][w]; segments: rows (x0, y0, x1, y1, palette index); markers: rows (x, y, palette index, r2); palette: rows
    (B, G, R) -> uint8 [h][w][channels]"""
    h, w = gray.shape
    out = np.empty((h, w, channels), np.uint8)
    for c in range(3):
        out[:, :, c] = gray
    if channels == 4:
        out[:, :, 3] = 255
    pal = [tuple(int(v) for v in p) for p in palette]
    for s in segments:
        x0, y0, x1, y1, pi = (int(v) for v in s)
        for x, y in _clipped_segment(x0, y0, x1, y1, w, h):
            out[y, x, 0], out[y, x, 1], out[y, x, 2] = pal[pi]
    for m in markers:
        x, y, pi, r2 = (int(v) for v in m)
        for px, py in marker_pixels(x, y, r2):
            if 0 <= px < w and 0 <= py < h:
                out[py, px, 0], out[py, px, 1], out[py, px, 2] = pal[pi]
    return out


# ---- the outer view (include/XRSLAM.h: XRSLAMAmdRenderTrackingView) from the feature list alone
VIEW_PALETTE = [(0, 255, 255), (0, 0, 255), (0, 255, 255), (0, 255, 0), (255, 255, 0), (255, 160, 0)]


def view_primitives(features, color_mode=0, draw_new=0, trail=0):
    """features: records with x, y, track_id, age, n_trail, trail (XRSLAMAmdGetFeatures) -> (segments, markers) over VIEW_PALETTE"""
    segs, new, tracked = [], [], []
    for f in features:
        x, y = int(f["x"]), int(f["y"])   # int() truncates, like .cast<int>()
        if f["track_id"] < 0:
            if draw_new:
                new.append((x, y, 4, 2))
            continue
        age = int(f["age"])
        tracked.append((x, y, (1 if age < 4 else 2 if age < 10 else 3) if color_mode == 1 else 0, 10))
        for j in range(min(int(trail), int(f["n_trail"]))):
            qx, qy = int(f["trail"][j][0]), int(f["trail"][j][1])
            segs.append((x, y, qx, qy, 5))
            x, y = qx, qy
    return segs, new + tracked
