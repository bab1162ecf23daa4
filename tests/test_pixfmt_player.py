"""xrslam-player --push-format on small synthetic ASL directories.

gray16: the frames are 16-bit PNGs (the scene's gray value in the high byte, seeded noise in the low byte).  Without the flag the
reader strips them to their high byte (player/euroc_io.hpp: decode_png); with it the 16-bit samples are handed to the library as
GRAY16, which keeps the high byte -- on the host in the CPU reference build, in the frame's upload on the GPU.  rgb / rgba: colour
PNGs pushed as RGB8 / RGBA8 instead of being reduced by the reader, same weights.  The TUM file must be byte-identical either way,
with the rectification in the library, in the player's reader, or off."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import pixfmt_model as pm

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
    low = np.random.RandomState(4).randint(0, 256, size=g.shape)
    roots = {"gray16": euroc.write_euroc(dict(seq, frames=((g.astype(np.uint16) << 8) | low.astype(np.uint16))), str(tmp_path / "g16" / "mav0"))}
    for name, fmt in (("rgb", pm.RGB8), ("rgba", pm.RGBA8)):
        roots[name] = euroc.write_euroc(dict(seq, frames=pm.encode(g, fmt)), str(tmp_path / name / "mav0"))
    return roots


def _tum(player, root, out, *extra):
    cmd = [player, "-sc", SLAM, "-dc", SENSOR, "--tum", out, "--bootstrap-frames", "60", "euroc://" + root] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["error"] == "" and res["frames"] == N, res
    with open(out, "rb") as fh:
        return fh.read(), res


def _check(player, tmp_path, modes):
    roots = _dirs(tmp_path)
    for name, root in roots.items():
        for k, mode in enumerate(modes if name == "gray16" else modes[:1]):
            plain, res = _tum(player, root, str(tmp_path / ("plain_%s_%d.tum" % (name, k))), *mode)
            pushed, _ = _tum(player, root, str(tmp_path / ("pushed_%s_%d.tum" % (name, k))), "--push-format", name, *mode)
            if "--no-undistort" in mode:                                # (the renderer does not distort: only this run tracks the scene)
                assert res["tracked"] >= 20 and plain.count(b"\n") == res["tracked"]
            assert pushed == plain, "%s, %s" % (name, mode)


def test_player_rejects_an_unknown_push_format(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    p = subprocess.run([PLAYER_REF, "-sc", SLAM, "-dc", SENSOR, "--push-format", "v210", "euroc://" + str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 2 and "--push-format" in p.stderr


def test_cpu_reference_player_push_format_writes_the_same_trajectory(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    _check(PLAYER_REF, tmp_path, [("--no-undistort",), ("--host-undistort",)])


@pytest.mark.gpu
def test_player_push_format_writes_the_same_trajectory(tmp_path):
    if not os.path.exists(PLAYER):
        pytest.fail("xrslam-player is not built (run __graft_entry__.build())")
    _check(PLAYER, tmp_path, [("--no-undistort",), (), ("--host-undistort",)])
