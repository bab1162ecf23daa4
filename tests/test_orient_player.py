"""xrslam-player --push-oriented on small synthetic ASL directories.

With --push-oriented O the reader turns every PNG by the inverse of orientation O -- the frame a sensor mounted that way delivers --
and sets XRSLAMAmdSetFrameOrientation(O); the library turns it back: on the host in the CPU reference build (pixel_format.hpp:
orient_plane), in the frame's upload on the GPU (k_orient).  The run sees the original images, so the TUM file must be byte-identical
to the plain run's -- through --push-scaled as well.  A name that is no orientation is a usage error."""
import json
import os
import subprocess

import pytest

from tests import scale_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAYER_REF = os.path.join(ROOT, "oracle", "_build", "xrslam-player-ref")
PLAYER = os.path.join(ROOT, "xrslam_amd", "bin", "xrslam-player")
SLAM = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR = os.path.join(ROOT, "configs", "euroc_sensor.yaml")
N = 64


def _dirs(tmp_path, full):
    from xrslam_amd.harness import euroc, scene
    seq = scene.make_sequence(n_frames=N, seed=5)
    g = seq["frames"]
    out = {"plain": euroc.write_euroc(seq, str(tmp_path / "plain" / "mav0"))}
    if full:
        out["big"] = euroc.write_euroc(dict(seq, frames=sm.replicate(g, 2, 2)), str(tmp_path / "big" / "mav0"))
    return out


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


def _check(player, tmp_path, mode, orientations, full):
    roots = _dirs(tmp_path, full)
    plain, res = _tum(player, roots["plain"], str(tmp_path / "plain.tum"), *mode)
    if "--no-undistort" in mode:                                # (the renderer does not distort: only this run tracks the scene)
        assert res["tracked"] >= 20 and plain.count(b"\n") == res["tracked"]
    for o in orientations:
        turned, _ = _tum(player, roots["plain"], str(tmp_path / ("turned_%s.tum" % o)), "--push-oriented", o, *mode)
        assert turned == plain, "--push-oriented %s, %s" % (o, mode)
    if full:
        scaled, _ = _tum(player, roots["big"], str(tmp_path / "scaled.tum"), "--push-scaled", "--push-oriented", "rot270", *mode)
        assert scaled == plain, "oversized frames, turned"
    # a name that is no orientation
    p = _play(player, roots["plain"], str(tmp_path / "refused.tum"), "--push-oriented", "rot45", *mode)
    assert p.returncode == 2 and "--push-oriented: rot90, rot180, rot270, flip" in p.stderr


def test_cpu_reference_player_push_oriented_writes_the_same_trajectory(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    _check(PLAYER_REF, tmp_path, ("--no-undistort",), ["rot90", "flip-rot180"], full=False)   # (a CPU run takes seconds: one of each class)


@pytest.mark.gpu
def test_player_push_oriented_writes_the_same_trajectory(tmp_path):
    if not os.path.exists(PLAYER):
        pytest.fail("xrslam-player is not built (run __graft_entry__.build())")
    _check(PLAYER, tmp_path, (), ["rot90", "flip"], full=True)   # (rectified on the device: turned first, rectified second)
