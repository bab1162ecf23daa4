#!/usr/bin/env python3
"""What a scaled upload costs: HIP-event time of xrhip_image_upload_scaled for 1920x1080 -> 752x480 through the crop
{114, 0, 1692, 1080} (GRAY8, the luma plane of NV12, BGR8) and for 3840x2160 GRAY8 (the whole frame as the crop), host source
(through the pinned slots and the HBM scratch) and HBM source.  Beside each: the plain 752x480 upload of the same format measured
in the same call, the source bytes over the HBM peak of profiles/r06_peaks.json (the traffic bound of the kernel's reads), and --
host case -- the bytes that cross the host link.

A figure is the time between two events on the context's stream (xrhip_debug_stream_span) around `--reps` back-to-back uploads,
divided by reps; median of `--rounds` rounds after a warm-up round; the cases alternate inside every round so that drift hits all
alike.  A host-source figure includes the CPU's copy of the crop into the pinned slot wherever that, and not the device, is what the
stream waits for.  Profilers off.  Every timed case is checked against tests/scale_model.py afterwards.  Writes a markdown table
(profiles/frame_scale.md holds one).

    tools/frame_scale.py --out bench_outputs/frame_scale.md"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "frame_scale.md"))
    args = ap.parse_args()
    import numpy as np

    from tests import color_frames as cf
    from tests import pixfmt_model as pm
    from tests import scale_model as sm
    from xrslam_amd import _lib, klt
    if _lib.device_count() < 1:
        raise SystemExit("frame_scale.py: no HIP device visible")
    _lib.set_device(0)
    with open(os.path.join(ROOT, "profiles", "r06_peaks.json")) as fh:
        peak_gbs = json.load(fh)["stream_read_gbs"]
    W, H = 752, 480
    hd = (1920, 1080, 114, 0, 1692, 1080)
    uhd = (3840, 2160, 0, 0, 3840, 2160)
    rows = [("1920x1080 gray8", pm.GRAY8, hd), ("1920x1080 nv12 luma", pm.NV12, hd), ("1920x1080 bgr8", pm.BGR8, hd), ("3840x2160 gray8", pm.GRAY8, uhd)]
    hbm = cf.Hbm()
    ctx = klt.KltContext(W, H, 150)
    im = ctx.image()
    cases = []
    for k, (name, fmt, geo) in enumerate(rows):
        bpp = pm.BYTES[fmt]
        px = cf.random_pixels(geo[0], geo[1], bpp, seed=k + 1)
        small = cf.random_pixels(W, H, bpp, seed=k + 11)
        cases.append(dict(name=name, fmt=fmt, geo=geo, bpp=bpp, px=px, dev=hbm.put(px), small=small, small_dev=hbm.put(small)))

    def run(c, what, src):
        if what == "scaled":
            if src == "host":
                im.upload_scaled(c["px"], c["geo"], c["fmt"])
            else:
                im.upload_scaled(c["dev"], c["geo"], c["fmt"], on_device=True, stride=c["px"].strides[0])
        elif src == "host":
            im.upload_format(c["small"], c["fmt"])
        else:
            im.upload_format(c["small_dev"], c["fmt"], on_device=True, stride=c["small"].strides[0])

    res = {}
    for rnd in range(args.rounds + 1):
        for ci, c in enumerate(cases):
            for what in ("scaled", "plain"):
                for src in ("host", "hbm"):
                    run(c, what, src)                      # (slots, scratch and caches as in a running stream)
                    ctx.stream_span(0)
                    for _ in range(args.reps):
                        run(c, what, src)
                    ms = ctx.stream_span(1)
                    if rnd:   # round 0 warms up
                        res.setdefault((ci, what, src), []).append(ms / args.reps * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    lines = ["Kernel revision `%s`, %d rounds of %d uploads, HBM read peak %.0f GB/s (profiles/r06_peaks.json)." % (_lib.kernel_revision(), args.rounds, args.reps, peak_gbs), "",
             "| frame -> 752x480 | crop bytes | scaled, host, us | scaled, HBM, us | plain 752x480, host, us | plain 752x480, HBM, us | crop bytes / HBM peak, us | bytes over the host link |",
             "|---|---|---|---|---|---|---|---|"]
    for ci, c in enumerate(cases):
        geo = c["geo"]
        run(c, "scaled", "hbm")                            # what was timed is the right plane
        np.testing.assert_array_equal(im.raw(), sm.scale(c["px"], geo, W, H, c["fmt"]))
        run(c, "scaled", "host")
        np.testing.assert_array_equal(im.raw(), sm.scale(c["px"], geo, W, H, c["fmt"]))
        crop_bytes = geo[4] * geo[5] * c["bpp"]
        lines.append("| %s | %d | %.1f | %.1f | %.1f | %.1f | %.2f | %d |" % (
            c["name"], crop_bytes, med[(ci, "scaled", "host")], med[(ci, "scaled", "hbm")], med[(ci, "plain", "host")], med[(ci, "plain", "hbm")],
            crop_bytes / (peak_gbs * 1e9) * 1e6, crop_bytes))
    ctx.synchronize()
    hbm.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
