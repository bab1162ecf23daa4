#!/usr/bin/env python3
"""What masks cost: (1) the per-frame detect and track times (HIP events, xrhip_klt_get_stats) of the S1 stream -- the synthetic
752x480 sequence of bench.py -- with no mask, with a static mask and with a per-frame mask resident in HBM, the three alternating over
`--rounds` rounds in one process so that drift hits all alike; (2) k_mask_ingest alone at 752x480 and 1280x720 (xrhip_debug_stream_span
around `--reps` back-to-back ingests of an HBM mask, median of the rounds).  Profilers off.  Writes a markdown table
(profiles/masks.md holds one).

    tools/masks.py --out bench_outputs/masks.md"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream(seq, mask_mode, mask, dev_mask, frames):
    """-> (detect us / frame, track us / frame, frames / s of the host loop) over the frames behind initialisation"""
    import time

    from xrslam_amd import _lib
    from xrslam_amd.harness import runner
    s = runner.Session(_lib.LIB_PATH, seq, instance=True)
    s.set_profiling(True)
    if mask_mode == "static":
        assert s.set_mask(mask), s.error()
    for _ in range(60):
        s.step()
    s.sync()
    s.klt_stats(reset=True)
    t0 = time.perf_counter()
    n = 0
    while n < frames:
        if mask_mode == "per_frame_hbm":
            assert s.set_next_frame_mask(dev_mask, on_device=True, stride=mask.shape[1]), s.error()
        if not s.step():
            break
        n += 1
    s.sync()
    dt = time.perf_counter() - t0
    st = s.klt_stats()
    s.close()
    return 1e3 * st.ms_detect / max(st.n_detect, 1), 1e3 * st.ms_track / max(st.n_track, 1), n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "masks.md"))
    args = ap.parse_args()
    import numpy as np

    from tests import color_frames as cf
    from xrslam_amd import _lib, klt
    from xrslam_amd.harness import scene
    if _lib.device_count() < 1:
        raise SystemExit("masks.py: no HIP device visible")
    _lib.set_device(0)
    hbm = cf.Hbm()
    seq = scene.make_sequence(n_frames=60 + args.frames, seed=1)
    h, w = seq["frames"][0].shape
    mask = np.full((h, w), 255, np.uint8)
    mask[:, :w // 3] = 0
    dev_mask = hbm.put(mask)
    modes = ("none", "static", "per_frame_hbm")
    got = {m: [] for m in modes}
    stream(seq, "none", mask, dev_mask, 20)   # warm-up
    for _ in range(args.rounds):
        for m in modes:
            got[m].append(stream(seq, m, mask, dev_mask, args.frames))
    lines = ["| S1 stream, %d frames behind initialisation | detect, us / frame | track, us / frame | host loop, frames / s |" % args.frames, "|---|---|---|---|"]
    for m in modes:
        cols = []
        for k in range(3):
            v = [r[k] for r in got[m]]
            cols.append("%.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v)))
        lines.append("| %s | %s |" % (m, " | ".join(cols)))
    lines += ["", "| k_mask_ingest alone, HBM source | us / launch |", "|---|---|"]
    for sw, sh in ((752, 480), (1280, 720)):
        ctx = klt.KltContext(sw, sh, 150)
        im = ctx.image(np.zeros((sh, sw), np.uint8))
        m = np.random.RandomState(1).choice(np.array([0, 255], np.uint8), size=(sh, sw))
        d = hbm.put(m)
        spans = []
        for r in range(args.rounds + 1):
            ctx.stream_span(0)
            for _ in range(args.reps):
                im.set_mask(d, on_device=True, stride=sw)
            spans.append(1e3 * ctx.stream_span(1) / args.reps)
        assert np.array_equal(im.mask(), (m != 0).astype(np.uint8))
        spans = spans[1:]
        lines.append("| %d x %d | %.2f (%.2f .. %.2f) |" % (sw, sh, statistics.median(spans), min(spans), max(spans)))
        im.close()
        ctx.close()
    hbm.close()
    text = "kernel revision `%s`\n\n" % _lib.kernel_revision() + "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
