"""What a tracking-view render costs (xrhip_image_render_view): HIP-event time per render at 752x480 with 150 markers, with and
without 8-segment trails, to a host and to an HBM destination, 200 renders behind 20 warm-up renders each; prints one JSON line
(profiles/tracking_view.md quotes it next to the frame time of the same build).  Usage: python tools/tracking_view.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(reps=200, warm=20):
    from tests.util import noise_image
    from tests.view_hbm import HbmOut
    from xrslam_amd import _lib, klt
    _lib.set_device(0)
    w, h = 752, 480
    r = np.random.RandomState(1)
    ctx = klt.KltContext(w, h, 150)
    im = ctx.image(noise_image(w, h, seed=3))
    pts = np.stack([r.randint(10, w - 10, 150), r.randint(10, h - 10, 150)], 1)
    mk = [(int(x), int(y), 0, 10) for x, y in pts]
    sg = []
    for x, y in pts:                      # eight segments of ~6 pixels behind every marker
        for _ in range(8):
            nx, ny = int(x + r.randint(-6, 7)), int(y + r.randint(-6, 7))
            sg.append((int(x), int(y), nx, ny, 1))
            x, y = nx, ny
    pal = [(0, 255, 255), (255, 160, 0)]
    hbm = HbmOut()
    dev = hbm.alloc(w * h * 4)
    host = np.zeros(w * h * 4, np.uint8)
    out = {"width": w, "height": h, "markers": len(mk), "trail_segments": len(sg), "renders": reps, "kernel_revision": _lib.kernel_revision()
           if hasattr(_lib, "kernel_revision") else None}
    for name, segs in (("markers", []), ("markers_trails", sg)):
        for ch in (3, 4):
            for dest in ("host", "hbm"):
                kw = dict(out=dev, on_device=True) if dest == "hbm" else dict(out=host)
                for _ in range(warm):
                    im.render_view(segs, mk, pal, ch, **kw)
                ctx.view_timing(1, reset=True)
                samples = []
                for _ in range(reps):
                    im.render_view(segs, mk, pal, ch, **kw)
                    samples.append(ctx.view_timing(-1, reset=True)[0])
                ctx.view_timing(0)
                s = np.array(samples) * 1e3
                out["%s_c%d_%s_us" % (name, ch, dest)] = {"median": round(float(np.median(s)), 2), "p10": round(float(np.percentile(s, 10)), 2),
                                                          "p90": round(float(np.percentile(s, 90)), 2)}
    hbm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
