#!/usr/bin/env python3
"""What a frame's upload costs per pixel format: microseconds per xrhip_image_upload_format at 752x480 and 1280x720, host source
(through the pinned slots) and HBM source, beside the gray and BGRA uploads, all in one process.  Each figure is a host clock around
`--reps` back-to-back uploads that end in a device synchronise, median of `--rounds` rounds after a warm-up round; the formats
alternate inside every round so that drift hits all alike.  Profilers off.  Writes a markdown table (profiles/pixel_formats.md
holds one).

    tools/pixel_formats.py --out bench_outputs/pixel_formats.md

--packed: instead, the packed 10 / 12-bit uploads (GRAY10_MIPI, GRAY12P, BAYER_RGGB10P) beside their 16-bit counterparts (GRAY16 and
BAYER_RGGB16, 12 bits) at 752x480, host and HBM source, and one scaled 1920x1080 -> 752x480 row each, as profiles/packed_formats.md
holds them: HIP-event time (xrhip_debug_stream_span) around 100 back-to-back uploads, median of 5 spans after a warm-up span, every
configuration compared with its model first.

    tools/pixel_formats.py --packed --out bench_outputs/packed_formats.md"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def packed(args):
    import numpy as np

    from tests import bayer_model as bm
    from tests import color_frames as cf
    from tests import packed_model as pk
    from tests import pixfmt_model as pm
    from tests import scale_model as sm
    from xrslam_amd import _lib, klt
    if _lib.device_count() < 1:
        raise SystemExit("pixel_formats.py: no HIP device visible")
    _lib.set_device(0)
    W, H = 752, 480
    reps, spans = 100, 5
    # (name, format, bits, its packing or None)
    rows = [("gray16 12 bits", pm.GRAY16, 12, None), ("gray10_mipi", 32, 0, pk.MIPI10), ("gray12p", 35, 0, pk.P12),
            ("bayer_rggb16 12 bits", bm.RGGB16, 12, None), ("bayer_rggb10p", 48, 0, pk.P10)]
    hbm = cf.Hbm()
    ctx = klt.KltContext(W, H, 150)
    im = ctx.image()
    lines = ["| frame | format | bytes a row | host source, us | HBM source, us |", "|---|---|---|---|---|"]
    for what, geo in (("752x480", None), ("1920x1080 -> 752x480", (1920, 1080, 0, 0, 1920, 1080))):
        sw, sh = (geo[0], geo[1]) if geo else (W, H)
        cases = []
        for name, fmt, bits, packing in rows:
            if packing is None:
                px = pm.samples16(np.random.RandomState(fmt).randint(0, 1 << bits, size=(sh, sw)))
                model = (sm.scale(px, geo, W, H, fmt, bits) if geo else pm.reduce(px, fmt, bits)) if fmt == pm.GRAY16 else \
                    (bm.scale(px, geo, W, H, fmt, bits) if geo else bm.reduce(px, fmt, bits))
            else:
                px = pk.pack(pk.random_samples(sw, sh, packing, seed=fmt), packing)
                model = pk.scale(px, geo, W, H, fmt) if geo else pk.reduce(px, sw, fmt)
            cases.append((name, fmt, bits, px, hbm.put(px), model))

        def upload(fmt, bits, px, dev, src):
            if geo:
                im.upload_scaled(px if src == "host" else dev, geo, fmt, bits, on_device=src == "hbm", stride=px.strides[0])
            else:
                im.upload_format(px if src == "host" else dev, fmt, bits, on_device=src == "hbm", stride=px.strides[0])
        res = {}
        for name, fmt, bits, px, dev, model in cases:   # every configuration against its model first
            for src in ("host", "hbm"):
                upload(fmt, bits, px, dev, src)
                np.testing.assert_array_equal(im.raw(), model, err_msg="%s, %s, %s" % (what, name, src))
        for rnd in range(spans + 1):
            for name, fmt, bits, px, dev, model in cases:
                for src in ("host", "hbm"):
                    ctx.synchronize()
                    ctx.stream_span(0)
                    for _ in range(reps):
                        upload(fmt, bits, px, dev, src)
                    ms = ctx.stream_span(1)
                    if rnd:   # span 0 warms up
                        res.setdefault((name, src), []).append(1e3 * ms / reps)
        for name, fmt, bits, px, dev, model in cases:
            med = {src: sorted(res[(name, src)])[len(res[(name, src)]) // 2] for src in ("host", "hbm")}
            lines.append("| %s | %s | %d | %.1f | %.1f |" % (what, name, px.strides[0], med["host"], med["hbm"]))
    ctx.synchronize()
    hbm.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true", help="the packed 10 / 12-bit uploads beside their 16-bit counterparts")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "pixel_formats.md"))
    args = ap.parse_args()
    if args.packed:
        return packed(args)
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
