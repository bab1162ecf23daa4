"""xrslam-player --push-format gray10_mipi | gray12_mipi | gray10p | gray12p | bayer_rggb10_mipi | bayer_bggr12p on small synthetic
ASL directories.

With the flag the player re-packs each gray PNG on the host into the rows a sensor would send -- a 16-bit PNG keeps its top 10 / 12
bits, an 8-bit one is shifted up -- and pushes them packed; the library unpacks them (on the host in the CPU reference build, in the
frame's upload on the GPU).  The top 8 bits of every sample are the PNG's high byte, so the TUM file must be byte-identical to the
run that pushes the same PNGs as --push-format gray16 (the mono forms) or as the unpacked mosaic of the same pattern (the Bayer forms:
every site holds the gray value) -- also through --push-scaled and --push-oriented."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import scale_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAYER_REF = os.path.join(ROOT, "oracle", "_build", "xrslam-player-ref")
PLAYER = os.path.join(ROOT, "xrslam_amd", "bin", "xrslam-player")
SLAM = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR = os.path.join(ROOT, "configs", "euroc_sensor.yaml")
N = 64
# (directory, packed --push-format, its twin's --push-format, further flags)
PLAN_REF = [("g16", "gray10_mipi", "gray16", ("--no-undistort",)),
            ("g16", "gray12p", "gray16", ("--host-undistort",)),
            ("g8", "bayer_rggb10_mipi", "bayer_rggb8", ("--no-undistort",)),
            ("g16x2", "gray12_mipi", "gray16", ("--no-undistort", "--push-scaled")),
            ("g16", "gray10p", "gray16", ("--no-undistort", "--push-oriented", "rot90"))]
PLAN_GPU = [("g16", "gray10_mipi", "gray16", ()),
            ("g16x2", "gray12p", "gray16", ("--no-undistort", "--push-scaled")),
            ("g8", "bayer_bggr12p", "bayer_bggr16", ("--no-undistort", "--push-oriented", "flip-rot90"))]


def _dirs(tmp_path, wanted):
    from xrslam_amd.harness import euroc, scene
    seq = scene.make_sequence(n_frames=N, seed=5)
    g = seq["frames"]
    low = np.random.RandomState(4).randint(0, 256, size=g.shape)
    g16 = (g.astype(np.uint16) << 8) | low.astype(np.uint16)
    frames = {"g16": lambda: g16, "g8": lambda: g, "g16x2": lambda: sm.replicate(g16, 2, 2)}
    return {k: euroc.write_euroc(dict(seq, frames=frames[k]()), str(tmp_path / k / "mav0")) for k in wanted}


def _tum(player, root, out, *extra):
    cmd = [player, "-sc", SLAM, "-dc", SENSOR, "--tum", out, "--bootstrap-frames", "60", "euroc://" + root] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["error"] == "" and res["frames"] == N, res
    with open(out, "rb") as fh:
        return fh.read(), res


def _check(player, tmp_path, plan):
    roots = _dirs(tmp_path, {p[0] for p in plan})
    twins = {}
    for k, (root, name, twin, flags) in enumerate(plan):
        if (root, twin, flags) not in twins:
            twins[(root, twin, flags)] = _tum(player, roots[root], str(tmp_path / ("twin_%d.tum" % k)), "--push-format", twin, *flags)
        plain, res = twins[(root, twin, flags)]
        pushed, _ = _tum(player, roots[root], str(tmp_path / ("packed_%d.tum" % k)), "--push-format", name, *flags)
        if "--no-undistort" in flags:                                # (the renderer does not distort: only this run tracks the scene)
            assert res["tracked"] >= 20 and plain.count(b"\n") == res["tracked"]
        assert pushed == plain, "%s against %s, %s" % (name, twin, flags)


def test_cpu_reference_player_push_format_packed_writes_the_same_trajectory(tmp_path):
    """(--host-undistort: the player's reader unpacks with the library's host formulas before it rectifies)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    _check(PLAYER_REF, tmp_path, PLAN_REF)


@pytest.mark.gpu
def test_player_push_format_packed_writes_the_same_trajectory(tmp_path):
    """Unpacked in the frame's upload: rectified by the library behind it (the default), unrectified, scaled and turned."""
    if not os.path.exists(PLAYER):
        pytest.fail("xrslam-player is not built (run __graft_entry__.build())")
    _check(PLAYER, tmp_path, PLAN_GPU)
