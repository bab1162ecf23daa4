"""The tracking view through the outer C API (include/XRSLAM.h) on the S1 stream: the feature snapshot against the 'F' records of the
output log (tests/outlog.py), the rendered view against tests/view_model.py applied to the pushed frame and primitives built from
XRSLAMAmdGetFeatures alone, the output log against the log of the same run that never asks for anything, XRSLAM_RESULT_FEATURES
through a compiled C++ host, and the player's --view-out.  Everything is assert_array_equal / byte equality."""
import json
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

from tests import outlog
from tests import view_model as vm
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_YAML = os.path.join(ROOT, "configs", "bench_slam_150.yaml")   # feature_tracker.max_frames 20 >= the history asked for
SENSOR_YAML = os.path.join(ROOT, "configs", "euroc_sensor.yaml")
PLAYER = os.path.join(ROOT, "xrslam_amd", "bin", "xrslam-player")
N = 40
HISTORY = 4


@pytest.fixture(scope="module")
def seq():
    q = scene.make_sequence(n_frames=N, seed=1, workers=max(1, min(8, len(os.sched_getaffinity(0)))))
    q["frames"].setflags(write=False)
    return q


def _session(seq, mode=0, group=None, instance=False):
    from xrslam_amd import _lib
    fd, path = tempfile.mkstemp(prefix="xr_view_", suffix=".bin")
    os.close(fd)
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path
    try:
        s = runner.Session(_lib.LIB_PATH, seq, slam_yaml=BENCH_YAML, threading=mode, instance=instance or group is not None, group=group)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
    return s, path


def _finish(s, path):
    s.flush()
    s.sync()
    assert not s.error(), s.error()
    s.close()
    with open(path, "rb") as fh:
        blob = fh.read()
    F, _ = outlog.read(path)
    os.unlink(path)
    return blob, F


def _plain_loop(s, path):
    while s.step():
        pass
    return _finish(s, path)


def _plain_run(seq, **kw):
    return _plain_loop(*_session(seq, **kw))


def _viewed_run(seq, **kw):
    return _viewed_loop(seq, *_session(seq, **kw))


def _viewed_loop(seq, s, path):
    """The run that looks at everything after every frame -> (log bytes, F records, [(t, features)] per newly tracked frame)"""
    s.set_feature_history(HISTORY)
    seen, last_t = [], None
    frame_of = {float(t): k for k, t in enumerate(seq["cam_t"])}
    while s.step():
        t, f = s.features()
        if t is None or t == last_t:
            continue
        last_t = t
        seen.append((t, f.copy()))
        g = seq["frames"][frame_of[t]]
        ref = s.render_view(3)
        assert ref is not None, s.error()
        np.testing.assert_array_equal(ref, vm.render(g, *vm.view_primitives(f), vm.VIEW_PALETTE, 3), err_msg="reference view, t = %r" % t)
        full = s.render_view(4, color_mode=1, draw_new=1, trail=HISTORY, stride=g.shape[1] * 4 + 12)
        assert full is not None, s.error()
        segs, mk = vm.view_primitives(f, 1, 1, HISTORY)
        np.testing.assert_array_equal(full, vm.render(g, segs, mk, vm.VIEW_PALETTE, 4), err_msg="age + new + trail view, t = %r" % t)
    blob, F = _finish(s, path)
    return blob, F, seen


def _check_features(F, seen):
    by_t = {r["t"]: k for k, r in enumerate(F)}
    assert len(seen) >= N - 2
    first, trails, tracked = {}, 0, 0
    for k, rec in enumerate(F):
        for tid in rec["track"][rec["track"] >= 0]:
            first.setdefault(int(tid), k)
    for t, f in seen:
        k = by_t[t]
        rec = F[k]
        np.testing.assert_array_equal(np.stack([f["x"], f["y"]], 1), rec["px"], err_msg="positions, t = %r" % t)
        np.testing.assert_array_equal(f["track_id"], rec["track"], err_msg="track ids, t = %r" % t)
        assert (f["age"][f["track_id"] < 0] == 0).all() and (f["n_trail"][f["track_id"] < 0] == 0).all()
        for e in f[f["track_id"] >= 0]:
            tid, age = int(e["track_id"]), int(e["age"])
            tracked += 1
            # a track shows its id from its second key point on, and grows by one per frame: that is its age (non-decreasing) until
            # the tracking map trims -- it keeps feature_tracker.max_frames = 20 frames once the system is initialised
            full = k - first[tid] + 2
            assert age == full if full <= 20 else 20 <= age <= full, "track %d at frame %d: age %d, key points so far %d" % (tid, k, age, full)
            assert e["n_trail"] == min(HISTORY, age - 1)
            for j in range(int(e["n_trail"])):
                prev = F[k - 1 - j]
                hit = np.flatnonzero((prev["px"] == e["trail"][j]).all(1))
                assert len(hit) == 1, "trail[%d] of track %d is not a key point of the frame %d back" % (j, tid, j + 1)
                # the same track there -- or none yet: a track gets its id when the NEXT frame continues the point
                assert prev["track"][hit[0]] == tid or (prev["track"][hit[0]] == -1 and j == full - 2)
                trails += 1
    assert tracked > 20 * len(seen) and trails > 2 * tracked


def test_before_the_first_frame(seq):
    """No features, and a view that says why it cannot be drawn; the frames that follow are tracked and viewed as usual."""
    s, path = _session(seq, instance=True)
    t0, f0 = s.features()
    assert t0 is None and len(f0) == 0
    assert s.render_view() is None and "no frame has been tracked" in s.error()
    assert s.step() and s.step() and s.step()
    t, f = s.features()
    assert t == float(seq["cam_t"][1]) and len(f) > 20
    assert s.render_view(4) is not None
    s.close()
    os.unlink(path)


@pytest.mark.parametrize("mode", [0, 1], ids=["inline", "pipelined"])
def test_solo_stream(seq, mode):
    want, Fw = _plain_run(seq, mode=mode)
    got, F, seen = _viewed_run(seq, mode=mode)
    assert len(Fw) == N
    assert got == want, "asking for features and views changed the output log (%d vs %d bytes)" % (len(got), len(want))
    _check_features(F, seen)


def test_member_of_a_group(seq):
    from xrslam_amd import _lib
    want, _ = _plain_run(seq, instance=True)
    group = runner.Group(_lib.LIB_PATH)
    res, errs = {}, []
    sv, sp = _session(seq, group=group), _session(seq, group=group)   # (created here: the log's path travels in the environment)

    def viewed():
        try:
            res["viewed"] = _viewed_loop(seq, *sv)
        except BaseException as e:   # noqa: BLE001
            errs.append(repr(e))

    def plain():
        try:
            res["plain"] = _plain_loop(*sp)
        except BaseException as e:   # noqa: BLE001
            errs.append(repr(e))
    th = [threading.Thread(target=viewed), threading.Thread(target=plain)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    group.close()
    assert not errs, errs
    assert res["viewed"][0] == want and res["plain"][0] == want
    _check_features(res["viewed"][1], res["viewed"][2])


def _blob(seq, path):
    fr = np.ascontiguousarray(seq["frames"])
    with open(path, "wb") as fh:
        fh.write(np.array([len(fr), fr.shape[2], fr.shape[1], len(seq["imu"])], np.int32).tobytes())
        fh.write(np.ascontiguousarray(seq["cam_t"], np.float64).tobytes())
        fh.write(np.ascontiguousarray(seq["imu"], np.float64).tobytes())
        fh.write(fr.tobytes())


def test_result_features_through_a_cpp_host(seq, tmp_path):
    """XRSLAM_RESULT_FEATURES (a std::vector) read by tests/host_check/view_features_host.cpp equals the tracked subset of the C getter."""
    from xrslam_amd import _lib
    exe = str(tmp_path / "view_features_host")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "host_check", "view_features_host.cpp"),
                           "-o", exe, "-L" + libdir, "-lxrslam_hip", "-Wl,-rpath," + libdir])
    short = {k: (v[:20] if k in ("frames", "cam_t", "states") else v) for k, v in seq.items()}
    blob = str(tmp_path / "frames.bin")
    _blob(short, blob)
    p = subprocess.run([exe, BENCH_YAML, SENSOR_YAML, blob], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert lines[0] == "before 0 0"
    frames, cur = [], None
    for ln in lines[1:]:
        tok = ln.split()
        if tok[0] == "frame":
            cur = {"n": int(tok[2]), "tracked": int(tok[3]), "size": int(tok[4]), "R": [], "G": []}
            frames.append(cur)
        elif tok[0] in ("R", "G"):
            cur[tok[0]].append((tok[1], tok[2]))
    assert len(frames) == 20
    for fr in frames:
        assert fr["size"] == fr["tracked"] == len(fr["R"]) and fr["R"] == fr["G"] and fr["n"] >= fr["tracked"]
    assert frames[0]["n"] == 0 and sum(fr["tracked"] for fr in frames) > 20 * 15


def _read_ppm(path):
    with open(path, "rb") as fh:
        data = fh.read()
    magic, dims, maxv, body = data.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert magic == b"P6" and maxv == b"255" and len(body) == w * h * 3
    return np.frombuffer(body, np.uint8).reshape(h, w, 3)


def test_player_view_out(seq, tmp_path):
    """--view-out DIR --view-every 5: one P6 file per fifth tracked frame, named by its timestamp in ns; a decoded file (RGB) equals
    XRSLAMAmdRenderTrackingView (BGR) of that frame in a session fed the same frames."""
    from xrslam_amd.harness import euroc
    if not os.path.exists(PLAYER):
        pytest.fail("xrslam-player is not built (run __graft_entry__.build())")
    n = 24
    short = {k: (v[:n] if k in ("frames", "cam_t", "states") else v) for k, v in seq.items()}
    root = euroc.write_euroc(short, str(tmp_path / "mav0"))
    # what the player reads back: time stamps through the file's integer nanoseconds, IMU rows up to 20 ms past the last image
    ns = lambda t: np.round(np.asarray(t, np.float64) * 1e9) * 1e-9   # noqa: E731
    imu = short["imu"][short["imu"][:, 0] <= float(short["cam_t"][-1]) + 0.02].copy()
    imu[:, 0] = ns(imu[:, 0])
    short = dict(short, cam_t=ns(short["cam_t"]), imu=imu)
    views = tmp_path / "views"
    views.mkdir()
    cmd = [PLAYER, "-sc", BENCH_YAML, "-dc", SENSOR_YAML, "--bootstrap-frames", "60", "--no-undistort", "--view-out", str(views),
           "--view-every", "5", "--view-mode", "age", "--view-trail", "3", "euroc://" + root]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["error"] == "" and res["frames"] == n
    files = sorted(os.listdir(str(views)), key=lambda s: int(s.split(".")[0]))
    tracked = n                                              # (the IMU file runs past the last image: every frame is tracked)
    assert res["views"] == len(files) == (tracked + 4) // 5, (res, files)
    want_names = ["%d.ppm" % int(round(float(t) * 1e9)) for t in short["cam_t"][:tracked:5]]
    assert files == want_names
    # the same frames through a session: the view of the frame behind the third file
    from xrslam_amd import _lib
    s = runner.Session(_lib.LIB_PATH, dict(short, frames=np.ascontiguousarray(short["frames"])), slam_yaml=BENCH_YAML)
    s.set_feature_history(3)
    target = float(short["cam_t"][10])
    got = None
    while s.step():
        t, _ = s.features()
        if t == target:
            got = s.render_view(3, color_mode=1, draw_new=1, trail=3)
            break
    s.close()
    assert got is not None
    np.testing.assert_array_equal(_read_ppm(str(views / files[2])), got[:, :, ::-1])
