#!/usr/bin/env python3
"""What colour input costs: frames/s of the S1 stream (752x480, configs/bench_slam_150.yaml) fed as gray host frames, BGR host,
BGRA host and BGRA resident in HBM, for one or more builds of the library, alternating between them inside one process-per-run
loop so that drift hits all builds alike.  Profilers off.  Writes a markdown table (profiles/color_input.md is one).

    tools/color_input.py --libs parent=path/to/old/libxrslam_hip.so this=xrslam_amd/lib/libxrslam_hip.so --frames 1000 --reps 3

A build without XRSLAMAmdPushImageDeviceColor (one that predates colour uploads) runs the three host inputs only: its colour
frames go through the host loop it has.  Every run is a child process (one HIP runtime, one library per process)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INPUTS = ("gray_host", "bgr_host", "bgra_host", "bgra_resident")


def child(args):
    import ctypes as C

    import numpy as np

    from xrslam_amd.harness import runner
    q = dict(np.load(args.stream))
    g = q["frames"]
    kind = args.child
    channels = {"gray_host": 1, "bgr_host": 3, "bgra_host": 4, "bgra_resident": 4}[kind]
    if channels == 1:
        frames = g
    else:
        g16 = g.astype(np.int16)
        planes = [g16, np.minimum(255, g16 + g16 // 8), g16 - g16 // 4] + ([np.full_like(g16, 255)] if channels == 4 else [])
        frames = np.ascontiguousarray(np.stack(planes, -1).astype(np.uint8))
    dev = None
    if kind == "bgra_resident":
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so.7")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(frames.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(frames.ctypes.data), C.c_size_t(frames.nbytes), 1) == 0
        dev = (p.value, frames.strides[0], frames.strides[1])
    s = runner.Session(args.lib, dict(q, frames=frames), slam_yaml=os.path.join(ROOT, "configs", "bench_slam_150.yaml"),
                       channels=channels, device_frames=dev)
    for _ in range(args.warmup):
        s.step()
    s.sync()
    t0 = time.perf_counter()
    n = 0
    while s.step():
        n += 1
    s.sync()
    dt = time.perf_counter() - t0
    err = s.error()
    tracked = len(s.poses)
    s.close()
    print(json.dumps({"input": kind, "frames": n, "seconds": dt, "fps": n / dt, "tracked": tracked, "error": err}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", default=["this=" + os.path.join(ROOT, "xrslam_amd", "lib", "libxrslam_hip.so")])
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inputs", nargs="+", default=list(INPUTS), choices=INPUTS)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "color_input.md"))
    ap.add_argument("--child")
    ap.add_argument("--lib")
    ap.add_argument("--stream")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import numpy as np

    from xrslam_amd.harness import scene
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    import tempfile
    stream = os.path.join(tempfile.mkdtemp(prefix="color_input_"), "stream.npz")
    q = scene.make_sequence(n_frames=args.frames + args.warmup, seed=1, workers=max(1, min(16, len(os.sched_getaffinity(0)))))
    np.savez(stream, **q)
    libs = [tuple(x.split("=", 1)) for x in args.libs]
    res = {}
    for rep in range(args.reps):
        for kind in args.inputs:
            for name, path in libs:   # the builds alternate inside every (repetition, input)
                if kind == "bgra_resident" and b"XRSLAMAmdPushImageDeviceColor" not in open(path, "rb").read():
                    continue
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--lib", path, "--stream", stream,
                                    "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    raise SystemExit("run failed (%s, %s): %s" % (name, kind, p.stderr[-2000:]))   # nothing more on the GPU after a failure
                r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                assert not r["error"] and r["frames"] == args.frames and r["tracked"] > 0.8 * args.frames, r
                res.setdefault((name, kind), []).append(r["fps"])
                print(name, kind, "%.1f frames/s" % r["fps"], flush=True)
    os.unlink(stream)
    lines = ["| build | input | frames/s (median) | min | max | ms/frame (median) | runs |", "|---|---|---|---|---|---|---|"]
    for name, _ in libs:
        for kind in INPUTS:
            v = sorted(res.get((name, kind), []))
            if v:
                med = v[len(v) // 2]
                lines.append("| %s | %s | %.1f | %.1f | %.1f | %.4f | %d |" % (name, kind, med, v[0], v[-1], 1e3 / med, len(v)))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
