"""xrslam-player --mask <file> on a small synthetic ASL directory: an 8-bit PGM (P5) or gray PNG at the working resolution becomes the
static mask before the first frame.  A file of another size is a start-up error that names both sizes (checked with the CPU reference
player: the loader runs before anything of the library); with an all-ones file the trajectory is the unmasked run's, byte for byte,
and with the left third hidden the player still tracks."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAYER_REF = os.path.join(ROOT, "oracle", "_build", "xrslam-player-ref")
PLAYER = os.path.join(ROOT, "xrslam_amd", "bin", "xrslam-player")
SLAM = os.path.join(ROOT, "configs", "bench_slam_150.yaml")
SENSOR = os.path.join(ROOT, "configs", "euroc_sensor.yaml")
W, H = 752, 480
N = 64


def _root(tmp_path):
    from xrslam_amd.harness import euroc, scene
    return euroc.write_euroc(scene.make_sequence(n_frames=N, seed=5), str(tmp_path / "seq" / "mav0"))


def _pgm(path, mask):
    with open(path, "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (mask.shape[1], mask.shape[0]) + mask.tobytes())
    return str(path)


def _play(player, root, out, *extra):
    cmd = [player, "-sc", SLAM, "-dc", SENSOR, "--tum", out, "--bootstrap-frames", "60", "--no-undistort", "euroc://" + root] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_a_mask_of_the_wrong_size_is_a_start_up_error(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    root = _root(tmp_path)
    p = _play(PLAYER_REF, root, str(tmp_path / "a.tum"), "--mask", _pgm(tmp_path / "small.pgm", np.ones((240, 320), np.uint8)))
    assert p.returncode == 1
    assert "the file is 320 x 240, the working resolution is 752 x 480" in p.stderr, p.stderr
    p = _play(PLAYER_REF, root, str(tmp_path / "b.tum"), "--mask", str(tmp_path / "missing.pgm"))
    assert p.returncode == 1 and "cannot open" in p.stderr
    # the CPU reference build has no masks: a good file is refused with the library's reason, not ignored
    p = _play(PLAYER_REF, root, str(tmp_path / "c.tum"), "--mask", _pgm(tmp_path / "ones.pgm", np.ones((H, W), np.uint8)))
    assert p.returncode == 1 and "not supported" in p.stderr, p.stderr


@pytest.mark.gpu
def test_player_mask(tmp_path):
    from PIL import Image
    if not os.path.exists(PLAYER):
        pytest.fail("xrslam-player is not built (run __graft_entry__.build())")
    root = _root(tmp_path)

    def tum(name, *extra):
        p = _play(PLAYER, root, str(tmp_path / name), *extra)
        assert p.returncode == 0, p.stdout + p.stderr
        res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        assert res["error"] == "" and res["frames"] == N, res
        with open(tmp_path / name, "rb") as fh:
            return fh.read(), res

    plain, res = tum("plain.tum")
    assert res["tracked"] >= 20
    ones, _ = tum("ones.tum", "--mask", _pgm(tmp_path / "ones.pgm", np.full((H, W), 255, np.uint8)))
    assert ones == plain
    m = np.full((H, W), 255, np.uint8)
    m[:, :W // 3] = 0
    Image.fromarray(m).save(str(tmp_path / "third.png"))
    third, res = tum("third.tum", "--mask", str(tmp_path / "third.png"))
    assert res["tracked"] >= 20 and third != plain
    p = _play(PLAYER, root, str(tmp_path / "bad.tum"), "--mask", _pgm(tmp_path / "small.pgm", np.ones((240, 320), np.uint8)))
    assert p.returncode == 1 and "320 x 240" in p.stderr and "752 x 480" in p.stderr
