"""CPU: the covariance entry points where there is no GPU.  The CPU reference build (the host sources over the oracle, no
xrhip_ba_covariance behind them) answers status -1 and says why; the player's --cov-out writes well-formed lines; every declared
symbol is exported; the host-only pieces (argument checks, the pose_ros permutation) pass a stand-alone program under the sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import lk_params_yaml as ly
from xrslam_amd.harness import runner, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "libxrslam_oracle.so")
PLAYER_REF = os.path.join(ROOT, "oracle", "_build", "xrslam-player-ref")
N, W, H = 40, 320, 240


@pytest.fixture(scope="module")
def oracle_lib():
    if not os.path.exists(ORACLE_LIB) or not os.path.exists(PLAYER_REF):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return ORACLE_LIB


@pytest.fixture(scope="module")
def seq():
    return scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))


def test_symbols_are_exported(oracle_lib):
    from xrslam_amd import _lib
    outer = ["XRSLAMAmdSetCovariance", "XRSLAMAmdGetCovariance", "XRSLAMAmdGetLandmarkVariances", "XRSLAMAmdInstanceSetCovariance",
             "XRSLAMAmdInstanceGetCovariance", "XRSLAMAmdInstanceGetLandmarkVariances"]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    product, ref = C.CDLL(_lib.LIB_PATH), C.CDLL(oracle_lib)
    for name in outer + ["xrhip_ba_covariance", "xrhip_ba_debug_cov_times"]:
        assert hasattr(product, name), name
    for name in outer:
        assert hasattr(ref, name), name
    assert not hasattr(ref, "xrhip_ba_covariance")   # weak and undefined there: the pipeline answers status -1
    assert C.sizeof(runner.XRSLAMAmdCovariance) == 8 * (1 + 225 + 36 + 1 + 1)


def test_cpu_reference_build_answers_status_minus_one(oracle_lib, seq):
    s = runner.Session(oracle_lib, seq, slam_yaml=ly.BENCH_YAML, sensor_yaml=ly.SENSOR_320, instance=True)
    ok, c = s.covariance()
    assert not ok and c.status == -1   # before anything ran
    s.set_covariance(True)
    while s.step():
        pass
    s.flush()
    s.sync()
    assert s.times().keyframes >= 1
    ok, c = s.covariance()
    assert not ok and c.status == -1 and not np.any(np.array(c.state))
    assert "no xrhip_ba_covariance" in s.error()
    var, ids = s.landmark_variances()
    assert len(var) == 0 and len(ids) == 0
    s.close()


def test_player_cov_out_writes_well_formed_lines(oracle_lib, seq, tmp_path):
    from xrslam_amd.harness import euroc
    root = euroc.write_euroc(seq, str(tmp_path / "mav0"))   # the synthetic stream as an EuRoC folder
    out = tmp_path / "cov.txt"
    p = subprocess.run([PLAYER_REF, "--slam", ly.BENCH_YAML, "--device", ly.SENSOR_320, "--euroc", str(root), "--bootstrap-frames", str(N),
                        "--no-undistort", "--cov-out", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = out.read_text().splitlines()
    assert len(lines) >= 1   # (this build has no covariance: every line says -1; the product build's lines: tests/test_cov_stream_gpu.py)
    for ln in lines:
        f = ln.split()
        assert len(f) == 23
        [float(v) for v in f[:22]]
        assert int(f[22]) in (-1, 0, 1, 2)


def test_host_pieces_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++ here")
    exe = str(tmp_path / "cov_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_check", "cov_host.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "cov_host OK" in p.stdout, p.stdout + p.stderr
