#!/usr/bin/env python3
"""What a frame's upload costs per pixel format: microseconds per xrhip_image_upload_format at 752x480 and 1280x720, host source
(through the pinned slots) and HBM source, beside the gray and BGRA uploads, all in one process.  Each figure is a host clock around
`--reps` back-to-back uploads that end in a device synchronise, median of `--rounds` rounds after a warm-up round; the formats
alternate inside every round so that drift hits all alike.  Profilers off.  Writes a markdown table (profiles/pixel_formats.md
holds one).

    tools/pixel_formats.py --out bench_outputs/pixel_formats.md"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "pixel_formats.md"))
    args = ap.parse_args()
    import numpy as np

    from tests import color_frames as cf
    from tests import pixfmt_model as pm
    from xrslam_amd import _lib, klt
    if _lib.device_count() < 1:
        raise SystemExit("pixel_formats.py: no HIP device visible")
    _lib.set_device(0)
    rows = [("gray8", pm.GRAY8, 0, 0), ("bgra8", pm.BGRA8, 0, 0), ("rgb8", pm.RGB8, 0, 0), ("rgba8", pm.RGBA8, 0, 0), ("gray16", pm.GRAY16, 16, 0),
            ("gray16 10 bits", pm.GRAY16, 10, 0), ("yuyv", pm.YUYV, 0, 0), ("uyvy limited", pm.UYVY, 0, 1), ("nv12", pm.NV12, 0, 0),
            ("nv12 limited", pm.NV12, 0, 1), ("p010", pm.P010, 0, 0)]
    hbm = cf.Hbm()
    lines = ["| size | format | bytes read | host source, us | HBM source, us |", "|---|---|---|---|---|"]
    for w, h in ((752, 480), (1280, 720)):
        ctx = klt.KltContext(w, h, 150)
        im = ctx.image()
        cases = []
        for name, fmt, bits, lim in rows:
            px = cf.random_pixels(w, h, pm.BYTES[fmt], seed=fmt + 1)
            cases.append((name, fmt, bits, lim, px, hbm.put(px)))
        res = {}
        for rnd in range(args.rounds + 1):
            for name, fmt, bits, lim, px, dev in cases:
                for src in ("host", "hbm"):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        if src == "host":
                            im.upload_format(px, fmt, bits, lim)
                        else:
                            im.upload_format(dev, fmt, bits, lim, on_device=True, stride=px.strides[0])
                    ctx.synchronize()
                    if rnd:   # round 0 warms up
                        res.setdefault((name, src), []).append((time.perf_counter() - t0) / args.reps * 1e6)
        for name, fmt, bits, lim, px, dev in cases:
            im.upload_format(dev, fmt, bits, lim, on_device=True, stride=px.strides[0])   # what was timed is the right plane
            np.testing.assert_array_equal(im.raw(), pm.reduce(px, fmt, bits, lim))
            med = {src: sorted(res[(name, src)])[len(res[(name, src)]) // 2] for src in ("host", "hbm")}
            lines.append("| %dx%d | %s | %d | %.1f | %.1f |" % (w, h, name, px.nbytes, med["host"], med["hbm"]))
        ctx.synchronize()
    hbm.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
