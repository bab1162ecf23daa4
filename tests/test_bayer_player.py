"""xrslam-player --push-format bayer_rggb8 | bayer_bggr16 on a small synthetic ASL directory.

With the flag the player takes each gray PNG as a raw mosaic -- every site holds the gray value: bytes for bayer_rggb8, 16-bit
samples with the value in the high byte for bayer_bggr16 -- and pushes it raw; the library demosaics it (on the host in the CPU
reference build, in the frame's upload on the GPU).  A second directory holds the model's gray planes of those mosaics
(tests/bayer_model.py) and is played without the flag.  The TUM files must be byte-identical, with the rectification in the library,
in the player's reader, or off."""
import json
import os
import subprocess

import pytest

from tests import bayer_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAYER_REF = os.path.join(ROOT, "oracle", "_build", "xrslam-player-ref")
PLAYER = os.path.join(ROOT, "xrslam_amd", "bin", "xrslam-player")
SLAM = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR = os.path.join(ROOT, "configs", "euroc_sensor.yaml")
N = 64
PUSHED = {"bayer_rggb8": bm.RGGB8, "bayer_bggr16": bm.BGGR8}     # (16 significant bits: the sample is the high byte, the gray value)


def _dirs(tmp_path):
    from xrslam_amd.harness import euroc, scene
    seq = scene.make_sequence(n_frames=N, seed=5)
    g = seq["frames"]
    roots = {"mosaic": euroc.write_euroc(seq, str(tmp_path / "mosaic" / "mav0"))}
    for name, fmt in PUSHED.items():
        plane = bm.reduce(g[..., None], fmt)
        assert (plane != g).mean() > 0.3
        roots[name] = euroc.write_euroc(dict(seq, frames=plane), str(tmp_path / name / "mav0"))
    assert (bm.reduce(g[:1, ..., None], bm.RGGB8) != bm.reduce(g[:1, ..., None], bm.BGGR8)).any()
    return roots


def _tum(player, root, out, *extra):
    cmd = [player, "-sc", SLAM, "-dc", SENSOR, "--tum", out, "--bootstrap-frames", "60", "euroc://" + root] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["error"] == "" and res["frames"] == N, res
    with open(out, "rb") as fh:
        return fh.read(), res


def _check(player, tmp_path, plan):
    """plan: (--push-format name, the player's undistortion flags) pairs"""
    roots = _dirs(tmp_path)
    for k, (name, mode) in enumerate(plan):
        plain, res = _tum(player, roots[name], str(tmp_path / ("plain_%s_%d.tum" % (name, k))), *mode)
        pushed, _ = _tum(player, roots["mosaic"], str(tmp_path / ("pushed_%s_%d.tum" % (name, k))), "--push-format", name, *mode)
        if "--no-undistort" in mode:                                # (the renderer does not distort: only this run tracks the scene)
            assert res["tracked"] >= 20 and plain.count(b"\n") == res["tracked"]
        assert pushed == plain, "%s, %s" % (name, mode)


def test_cpu_reference_player_push_format_bayer_writes_the_same_trajectory(tmp_path):
    """(--host-undistort: the player's reader demosaics with the library's host formulas before it rectifies)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    _check(PLAYER_REF, tmp_path, [("bayer_rggb8", ("--no-undistort",)), ("bayer_rggb8", ("--host-undistort",)), ("bayer_bggr16", ("--no-undistort",))])


@pytest.mark.gpu
def test_player_push_format_bayer_writes_the_same_trajectory(tmp_path):
    """Demosaiced in the frame's upload: rectified by the library behind it (the default), and unrectified."""
    if not os.path.exists(PLAYER):
        pytest.fail("xrslam-player is not built (run __graft_entry__.build())")
    _check(PLAYER, tmp_path, [("bayer_rggb8", ()), ("bayer_bggr16", ("--no-undistort",))])
