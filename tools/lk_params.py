#!/usr/bin/env python3
"""HIP-event time per xrhip_image_track launch over the Lucas-Kanade parameters (xrhip_klt_set_lk_params).

At the reference's 21 / 3 / 30 / 0.01 both paths are measured: the specialised kernels and, with xrhip_debug_force_general_lk, the
kernels with runtime parameters.  Then a few other points.  Each point: a band-limited noise frame and its copy moved by (3, -2),
the corners the device detects on the first (up to 150), `--launches` tracking launches without a guess after `--warmup` unrecorded
ones; the figure is ms_track / n_track of xrhip_klt_get_stats (event pairs round the LK launch alone).

The table replaces the part of profiles/lk_params.md between the two `times` markers (the file is created if it is missing).  No
figure here is a pass condition of anything.

    python tools/lk_params.py [--launches 200] [--warmup 20] [--out profiles/lk_params.md]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEGIN, END = "<!-- times:begin -->", "<!-- times:end -->"
# (frame size, (win, max_level, max_count, epsilon), development switch)
POINTS = [
    ((752, 480), (21, 3, 30, 0.01), False),
    ((752, 480), (21, 3, 30, 0.01), True),
    ((752, 480), (15, 3, 30, 0.01), False),
    ((752, 480), (9, 5, 30, 0.01), False),
    ((752, 480), (5, 0, 30, 0.01), False),
    ((1280, 720), (21, 3, 30, 0.01), False),
    ((1280, 720), (21, 5, 30, 0.01), False),
    ((1280, 720), (9, 5, 30, 0.01), False),
]


def measure(klt, size, params, forced, launches, warmup):
    from tests.util import noise_image, shifted
    w, h = size
    g = noise_image(w, h, seed=21)
    g2 = shifted(g, 3, -2)
    ctx = klt.KltContext(w, h, 150)
    ctx.set_lk_params(*params)
    ctx.force_general_lk(forced)
    A, B = ctx.image(g), ctx.image(g2)
    A.preprocess()
    B.preprocess()
    kp = A.detect_keypoints(np.zeros((0, 2)), 150, 20.0)
    for _ in range(warmup):
        A.track_keypoints(B, kp)
    ctx.set_profiling(True)
    ctx.stats(reset=True)
    kept = 0
    for _ in range(launches):
        _, st = A.track_keypoints(B, kp)
        kept = int(st.sum())
    s = ctx.stats()
    row = dict(size="%dx%d" % size, params="%d / %d / %d / %g" % params, path="general" if (forced or params != klt.LK_DEFAULTS) else "specialised",
               points=len(kp), kept=kept, us=1000.0 * s.ms_track / max(1, s.n_track), templates=s.lk_templates / max(1, s.n_track),
               iterations=s.lk_iterations / max(1, s.n_track))
    A.close()
    B.close()
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk_params.md"))
    a = ap.parse_args()
    from xrslam_amd import _lib, klt
    rows = [measure(klt, size, params, forced, a.launches, a.warmup) for size, params, forced in POINTS]
    import torch
    box = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "unknown device"
    lines = [BEGIN, "", "Box: %s, kernel revision %s, %d launches per point after %d warm-up launches." % (box, _lib.kernel_revision(), a.launches, a.warmup),
             "", "| frame | win / max_level / max_count / epsilon | path | points | kept | us per track launch | templates per launch | iterations per launch |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %(size)s | %(params)s | %(path)s | %(points)d | %(kept)d | %(us).1f | %(templates).0f | %(iterations).0f |" % r)
    lines += ["", END]
    table = "\n".join(lines)
    print(table)
    text = open(a.out).read() if os.path.exists(a.out) else "# Lucas-Kanade parameters: measured\n\n%s\n%s\n" % (BEGIN, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + table + text[text.index(END) + len(END):]
    else:
        text = text.rstrip("\n") + "\n\n" + table + "\n"
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
