"""xrslam-player --push-scaled on small synthetic ASL directories.

The PNGs of one directory are the scene's 752x480 frames; those of the others hold every pixel replicated 2x2 (1504x960), as gray
and as RGB.  With --push-scaled the player pushes an oversized PNG at its own size, the whole frame as the crop, and the library
scales it down -- on the host in the CPU reference build, in the frame's upload on the GPU.  Replicated pixels scale back to the
original bits (tests/test_scale_model.py), so the TUM file must be byte-identical to the plain run's.  Without the flag an
oversized PNG stays the error it was."""
import json
import os
import subprocess

import pytest

from tests import pixfmt_model as pm
from tests import scale_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAYER_REF = os.path.join(ROOT, "oracle", "_build", "xrslam-player-ref")
PLAYER = os.path.join(ROOT, "xrslam_amd", "bin", "xrslam-player")
SLAM = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR = os.path.join(ROOT, "configs", "euroc_sensor.yaml")
N = 64


def _dirs(tmp_path):
    from xrslam_amd.harness import euroc, scene
    seq = scene.make_sequence(n_frames=N, seed=5)
    g = seq["frames"]
    big = sm.replicate(g, 2, 2)
    return {"plain": euroc.write_euroc(seq, str(tmp_path / "plain" / "mav0")),
            "gray": euroc.write_euroc(dict(seq, frames=big), str(tmp_path / "gray" / "mav0")),
            "rgb": euroc.write_euroc(dict(seq, frames=pm.encode(big, pm.RGB8)), str(tmp_path / "rgb" / "mav0")),
            "rgb_plain": euroc.write_euroc(dict(seq, frames=pm.encode(g, pm.RGB8)), str(tmp_path / "rgb_plain" / "mav0"))}


def _play(player, root, out, *extra):
    cmd = [player, "-sc", SLAM, "-dc", SENSOR, "--tum", out, "--bootstrap-frames", "60", "euroc://" + root] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def _tum(player, root, out, *extra):
    p = _play(player, root, out, *extra)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["error"] == "" and res["frames"] == N, res
    with open(out, "rb") as fh:
        return fh.read(), res


def _check(player, tmp_path, modes, full):
    roots = _dirs(tmp_path)
    for k, mode in enumerate(modes):
        plain, res = _tum(player, roots["plain"], str(tmp_path / ("plain_%d.tum" % k)), *mode)
        if "--no-undistort" in mode:                                # (the renderer does not distort: only this run tracks the scene)
            assert res["tracked"] >= 20 and plain.count(b"\n") == res["tracked"]
        scaled, _ = _tum(player, roots["gray"], str(tmp_path / ("scaled_%d.tum" % k)), "--push-scaled", *mode)
        assert scaled == plain, "gray, %s" % (mode,)
        if full:
            same, _ = _tum(player, roots["plain"], str(tmp_path / ("same_%d.tum" % k)), "--push-scaled", *mode)   # nothing to scale: the plain path
            assert same == plain
        plain_rgb, _ = _tum(player, roots["rgb_plain"], str(tmp_path / ("plain_rgb_%d.tum" % k)), "--push-format", "rgb", *mode)
        for how in (("--push-format", "rgb"), ("--push-color",))[:2 if full else 1]:   # RGB8 by the library; BGR8 of the reader's channel order
            scaled, _ = _tum(player, roots["rgb"], str(tmp_path / ("scaled_rgb_%d.tum" % k)), "--push-scaled", *how, *mode)
            assert scaled == plain_rgb, "rgb, %s, %s" % (how, mode)
    # without the flag: the error it was
    p = _play(player, roots["gray"], str(tmp_path / "refused.tum"), *modes[0])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]) if "{" in p.stdout else {"frames": 0}
    assert "image is 1504x960, the device configuration says 752x480" in p.stderr and res["frames"] == 0


def test_cpu_reference_player_push_scaled_writes_the_same_trajectory(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    _check(PLAYER_REF, tmp_path, [("--no-undistort",)], full=False)   # (a CPU run takes seconds: the fewest that cover the flag)


@pytest.mark.gpu
def test_player_push_scaled_writes_the_same_trajectory(tmp_path):
    if not os.path.exists(PLAYER):
        pytest.fail("xrslam-player is not built (run __graft_entry__.build())")
    _check(PLAYER, tmp_path, [()], full=True)   # (rectified on the device: scaled first, rectified second)
