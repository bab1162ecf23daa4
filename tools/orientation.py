#!/usr/bin/env python3
"""What a turned upload costs: HIP-event time of one frame's upload per orientation class -- none (0), reversing (2: half a turn),
transposing (1: a quarter turn, the LDS tile) -- for 8-bit gray frames of 752x480 and 1280x720 from host memory and from HBM, and
for a 1920x1080 frame cropped and scaled to 752x480.  The unturned push stands beside every turned one, measured in the same round
of the same build; run with XRSLAM_HIP_LIB pointing at an earlier build's library (which has no orientation) the tool times the
unturned pushes alone, and --unturned-only does the same on this build, for the comparison across builds (a host-source figure
depends on how many other host frames pass through the CPU's caches in a round: compare like with like).

A figure is the time between two events on the context's stream (xrhip_debug_stream_span) around `--reps` back-to-back uploads,
divided by reps; per case the median of `--rounds` rounds after a warm-up round, with the rounds' minimum and maximum as the spread;
the cases alternate inside every round so that drift hits all alike.  A host-source figure includes the CPU's copy into the pinned
slot wherever that, and not the device, is what the stream waits for.  Profilers off.  Every timed case is checked against
tests/orient_model.py afterwards.  Writes a markdown table (profiles/orientation.md holds one).

    tools/orientation.py --out bench_outputs/orientation.md"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = (("none", 0), ("reversing", 2), ("transposing", 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--unturned-only", action="store_true", help="time the unturned pushes alone: the cases an earlier build's library runs, "
                    "with the same number of host frames competing for the CPU's caches")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "orientation.md"))
    args = ap.parse_args()
    import numpy as np

    from tests import color_frames as cf
    from tests import orient_model as om
    from tests import scale_model as sm
    from xrslam_amd import _lib, klt
    if _lib.device_count() < 1:
        raise SystemExit("orientation.py: no HIP device visible")
    _lib.set_device(0)
    have = hasattr(_lib.lib(), "xrhip_klt_set_orientation")
    classes = CLASSES if have and not args.unturned_only else CLASSES[:1]
    hbm = cf.Hbm()
    cases = []   # (name, context, image, class name, o, source, upload())
    keep = []
    for W, H, geo_of in ((752, 480, None), (1280, 720, None), (752, 480, "1080p")):
        ctx = klt.KltContext(W, H, 150)
        im = ctx.image()
        keep.append((ctx, im))
        for cname, o in classes:
            fw, fh = om.turned_size(W, H, o)
            if geo_of:   # the crop of the turned plane's aspect, as tall as the frame
                cw = 1692 if not o & 1 else 690
                geo = (1920, 1080, (1920 - cw) // 2, 0, cw, 1080)
                g = np.random.RandomState(3 + o).randint(0, 256, size=(1080, 1920), dtype=np.uint8)
                want = om.orient(sm.scale_gray(g, geo, fw, fh), o)
                name = "1920x1080 -> 752x480"
            else:
                geo = None
                g = np.random.RandomState(3 + o).randint(0, 256, size=(fh, fw), dtype=np.uint8)
                want = om.orient(g, o)
                name = "%dx%d" % (W, H)
            dev = hbm.put(g)
            for src in ("host", "hbm"):
                def upload(im=im, g=g, dev=dev, geo=geo, src=src):
                    if geo is not None:
                        if src == "host":
                            im.upload_scaled(g, geo)
                        else:
                            im.upload_scaled(dev, geo, on_device=True, stride=g.strides[0])
                    elif src == "host":
                        im.upload(g)
                    else:
                        im.upload_device(dev, g.strides[0])
                cases.append(dict(name=name, ctx=ctx, im=im, cls=cname, o=o, src=src, upload=upload, want=want, pixels=W * H))

    def set_o(c):
        if have:
            c["ctx"].set_orientation(c["o"])

    res = {}
    for rnd in range(args.rounds + 1):
        for k, c in enumerate(cases):
            set_o(c)
            c["upload"]()                      # (slots, scratch and caches as in a running stream)
            c["ctx"].stream_span(0)
            for _ in range(args.reps):
                c["upload"]()
            ms = c["ctx"].stream_span(1)
            if rnd:   # round 0 warms up
                res.setdefault(k, []).append(ms / args.reps * 1e3)
    lines = ["Kernel revision `%s`, %d rounds of %d uploads; us per upload: median (min .. max of the rounds)." % (_lib.kernel_revision(), args.rounds, args.reps), "",
             "| frame | source | " + " | ".join("%s (o = %d)" % c for c in classes) + " | turned plane bytes read + written |", "|---|---|" + "---|" * (len(classes) + 1)]
    table = {}
    for k, c in enumerate(cases):
        set_o(c)
        c["upload"]()                          # what was timed is the right plane
        np.testing.assert_array_equal(c["im"].raw(), c["want"], err_msg="%s %s %s" % (c["name"], c["src"], c["cls"]))
        v = sorted(res[k])
        table.setdefault((c["name"], c["src"]), {})[c["cls"]] = "%.1f (%.1f .. %.1f)" % (v[len(v) // 2], v[0], v[-1])
        table[(c["name"], c["src"])]["bytes"] = 2 * c["pixels"]
    for (name, src), row in table.items():
        lines.append("| %s | %s | " % (name, src) + " | ".join(row[c[0]] for c in classes) + " | %d |" % row["bytes"])
    for ctx, _ in keep:
        if have:
            ctx.set_orientation(0)
        ctx.synchronize()
    hbm.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
