"""XRSLAMAmdSetCovariance / GetCovariance / GetLandmarkVariances through the outer C API on 60 frames of the small 320 x 240 synthetic
stream (the first 36 frames seed the window and its first window solve is answered at frame 40, so a 40-frame run has nothing to look
at; 60 frames see five window solves): switching the covariance on changes nothing the pipeline outputs; the answer changes exactly on
the steps that make a keyframe, carries that keyframe's timestamp and is the block of that frame; with the switch off nothing of it is
launched.

Which frame: the output log's B record of a keyframe step names the window after the step; its last entry is the newest keyframe
(the frame just processed, or -- manage_keyframe's "lifted" branch -- the subframe lifted in its place, which then carries the processed
frame as its subframe), and the F records give that frame's timestamp.

Landmark variances: XRSLAM_RESULT_LANDMARKS carries points without ids and lists EVERY valid track of the map, also tracks that were
not parameters of the window solve (their first frame is no keyframe, or they were constant there), so the count cannot equal it; the
documented set is "free in that solve and still valid".  The ids are held against the valid track ids of the same step's B record, and
values, order and the id of every value (through the landmark's world point) against xrhip_ba_covariance on the window problem the run dumped (XRSLAM_AMD_DUMP_BA), solved
again on a context of its own.  Tolerance of that comparison: 1e-6 relative -- the bound the suite holds two solves of one frozen
problem to (tests/test_ba_gpu.py); the two runs execute the same kernels on the same bytes, the figure printed is expected to be 0."""
import glob
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import lk_params_yaml as ly
from tests import outlog
from xrslam_amd.harness import runner, scene

pytestmark = pytest.mark.gpu

N, W, H = 60, 320, 240
PERM = [3, 4, 5, 0, 1, 2]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAYER = os.path.join(ROOT, "xrslam_amd", "bin", "xrslam-player")


@pytest.fixture(scope="module")
def seq():
    return scene.make_sequence(n_frames=N, seed=1, w=W, h=H, K=(195.0, 194.5, 160.0, 120.0))


def _run(seq, cov, group=None, touch=True, dump_dir=None):
    """-> dict(log bytes, F / B records, counts, klt / ba statistics, seen: per step (frame index, available, timestamp, state, pose_ros,
    status, rcond, variances, ids, keyframes so far))"""
    from xrslam_amd import _lib
    fd, path = tempfile.mkstemp(prefix="xr_cov_", suffix=".bin")
    os.close(fd)
    os.environ["XRSLAM_AMD_DUMP_OUT"] = path
    if dump_dir is not None:
        os.environ["XRSLAM_AMD_DUMP_BA"] = str(dump_dir)
    try:
        s = runner.Session(_lib.LIB_PATH, seq, slam_yaml=ly.BENCH_YAML, sensor_yaml=ly.SENSOR_320, instance=True, group=group)
    finally:
        del os.environ["XRSLAM_AMD_DUMP_OUT"]
        os.environ.pop("XRSLAM_AMD_DUMP_BA", None)
    if touch:
        s.set_covariance(cov)
    seen = []
    while s.step():
        assert not s.error(), s.error()
        if cov:
            ok, c = s.covariance()
            var, ids = s.landmark_variances()
            seen.append((s.frame_k - 1, ok, c.timestamp, np.array(c.state), np.array(c.pose_ros), c.status, c.rcond_estimate, var, ids,
                         int(s.times().keyframes)))
    s.flush()
    s.sync()
    t = s.times()
    k, b = s.klt_stats(), s.ba_stats()
    out = dict(seen=seen, counts=(t.frames, t.solves, t.solve_iterations, t.marginalizations, t.keyframes),
               klt=(k.n_preprocess, k.n_track, k.n_detect, k.lk_points, k.lk_templates, k.lk_iterations),
               ba=(b.n_solve_try, b.n_trials, b.n_tiny), cov_launches=b.n_cov_launches, poses=list(s.poses))
    s.close()
    with open(path, "rb") as fh:
        out["log"] = fh.read()
    out["F"], out["B"] = outlog.read(path)
    os.unlink(path)
    return out


def _keyframe_steps(run):
    """-> [(step record, B record of the keyframe it made, timestamp of the newest keyframe of the window after it)], after asserting
    that the answer changes on exactly the steps that make a keyframe and is the very same answer on every other step"""
    t_of = {f["id"]: f["t"] for f in run["F"]}
    kf_B = [b for b in run["B"] if b["keyframe"]]
    out, made, prev = [], 0, None
    for r in run["seen"]:
        dk = r[9] - made
        made = r[9]
        assert dk in (0, 1), "a step made %d keyframes" % dk
        if dk == 0:
            if prev is None:
                assert not r[1] and r[5] == -1 and not r[3].any()          # nothing answered before the first window solve
            else:
                assert r[1] == prev[1] and r[2] == prev[2] and r[5] == prev[5] and r[6] == prev[6]
                assert np.array_equal(r[3], prev[3]) and np.array_equal(r[7], prev[7]) and np.array_equal(r[8], prev[8])
        else:
            b = kf_B[len(out)]
            newest, subs = b["window"][-1]
            assert b["id"] == newest or b["id"] in subs, "the processed frame is neither the newest keyframe nor its subframe"
            assert r[1] and r[5] == 0, "no covariance on the step that made keyframe %d" % newest
            assert r[2] == t_of[newest], "covariance of t = %r, the newest keyframe %d has t = %r" % (r[2], newest, t_of[newest])
            assert prev is None or r[2] > prev[2]
            out.append((r, b, t_of[newest]))
        prev = r
    return out


@pytest.fixture(scope="module")
def off_run(seq):
    r = _run(seq, False, touch=False)   # a run that never heard of the feature
    assert r["counts"][0] == N and r["counts"][4] >= 3 and r["cov_launches"] == 0, r["counts"]
    return r


@pytest.fixture(scope="module")
def on_run(seq):
    return _run(seq, True)


def test_output_log_is_byte_identical_with_covariance_on(off_run, on_run):
    assert on_run["counts"] == off_run["counts"] and on_run["poses"] == off_run["poses"]
    assert on_run["log"] == off_run["log"], "the output log differs from the run without the covariance"
    assert on_run["cov_launches"] > 0


def test_switched_off_launches_nothing(seq, off_run):
    r = _run(seq, False)   # switched off explicitly
    assert r["cov_launches"] == 0 and r["klt"] == off_run["klt"] and r["ba"] == off_run["ba"] and r["log"] == off_run["log"]


def test_answer_belongs_to_the_newest_keyframe_and_stays(seq, on_run):
    steps = _keyframe_steps(on_run)
    assert len(steps) >= 3 and len(steps) == on_run["seen"][-1][9]
    lifted = [b["id"] for _, b, _ in steps if b["id"] != b["window"][-1][0]]
    print("keyframe steps: %d, of which through the lifted branch: %d" % (len(steps), len(lifted)))
    cam_t = [float(t) for t in seq["cam_t"]]
    for r, b, t_kf in steps:
        k, ok, t, state, ros, status, rcond, var, ids, _ = r
        assert t in cam_t and t <= cam_t[k]
        assert 0 < rcond <= 1
        assert np.array_equal(ros, state[np.ix_(PERM, PERM)])
        assert np.array_equal(state, state.T) and np.all(np.diag(state) > 0)
        # the ids: unique, and ids of tracks that are valid after this step (the set XRSLAM_RESULT_LANDMARKS draws from)
        valid = set(b["track_id"][(b["track_tags"] >> outlog.TT_VALID) & 1 == 1].tolist())
        assert len(var) > 0 and np.all(var > 0) and len(set(ids.tolist())) == len(ids)
        assert set(ids.tolist()) <= valid and len(ids) <= len(valid)


def _landmark_point(pd, l):
    """World point of landmark l of a solved problem: its reference frame's camera pose, the reference bearing, the inverse depth.
    (slide_window re-anchors a track whose first frame leaves the window: then the log's inverse depth is another and the point moves
    by a reprojection error.)"""
    from tests.ba_synth import qmul, qrot
    o = int(np.flatnonzero(pd.obs_lm == l)[0])
    st = pd.frame_state[pd.obs_ref[o]]
    qc, pc = qmul(st[0:4], pd.cam_ext[0:4]), st[4:7] + qrot(st[0:4], pd.cam_ext[4:7])
    return pc + qrot(qc, pd.obs_z_ref[o]) / pd.inv_depth[l]


def test_blocks_and_variances_are_those_of_the_dumped_window_problem(seq, tmp_path):
    """Every window problem of a run is dumped, solved again on a context of its own and handed to xrhip_ba_covariance: the pipeline's
    block is the block of that problem's LAST frame (and of no other), its variances are those of the problem's free landmarks in the
    problem's order, and each carries the id of the track whose world point the log shows for it."""
    from tests import ba_snapshots
    from xrslam_amd import ba
    run = _run(seq, True, dump_dir=tmp_path)
    steps = _keyframe_steps(run)
    windows = [d for d in (ba_snapshots.read_xrba(p) for p in sorted(glob.glob(str(tmp_path / "ba_*.xrba")))) if len(d["prior_frames"])]
    assert len(steps) >= 3 and len(windows) >= len(steps)   # (the flush after the last step may solve one more window)
    ctx = ba.BaContext()
    worst, anchored = 0.0, 0
    for (r, b, _), d in zip(steps, windows):
        pd = ba_snapshots.to_problem(d)
        assert ctx.solve(pd).usable
        F = len(pd.frame_state)
        out = ctx.covariance(pd, np.arange(F), landmarks=True)
        assert out["status"] == 0
        err = [np.linalg.norm(r[3] - blk) / np.linalg.norm(blk) if blk.any() else np.inf for blk in out["blocks"]]
        worst = max(worst, err[F - 1])
        assert err[F - 1] <= 1e-6 and min(err[:F - 1]) > 1e-3, err   # (no two frames of a window share a covariance to three digits)
        # the variances: a subsequence of the problem's free landmarks, in its order
        point_of = dict(zip(b["track_id"].tolist(), b["point"]))
        depth_of = dict(zip(b["track_id"].tolist(), b["inv_depth"].tolist()))
        points = np.array([_landmark_point(pd, k) if (pd.obs_lm == k).any() else np.full(3, 1e30) for k in range(len(pd.inv_depth))])
        l = 0
        for v, tid in zip(r[7], r[8]):
            while l < len(out["var"]) and not (pd.landmark_fix[l] == 0 and abs(out["var"][l] - v) <= 1e-6 * v):
                l += 1
            assert l < len(out["var"]), "variance %r of track %d is none of the problem's (in order)" % (v, tid)
            # the track's world point in the log is landmark l's: exactly, while the track keeps its first frame; once slide_window
            # has re-anchored it (another inverse depth in the log) the point is rebuilt along the NEW first frame's bearing and moves by
            # that observation's reprojection error, which the landmark sweep bounds by 3 pixels (fx = 195) -- and l is the nearest landmark
            dist = np.linalg.norm(points - point_of[int(tid)], axis=1)
            same_anchor = abs(depth_of[int(tid)] - pd.inv_depth[l]) <= 1e-6 * abs(pd.inv_depth[l])
            anchored += int(same_anchor)
            bound = 1e-6 * np.linalg.norm(points[l]) if same_anchor else 3.0 / 195.0 / pd.inv_depth[l]
            assert int(np.argmin(dist)) == l and dist[l] <= bound, "track %d does not carry landmark %d (%g)" % (tid, l, dist[l])
            worst = max(worst, abs(out["var"][l] - v) / v)
            l += 1
    print("pipeline against the dumped problems: largest relative deviation %.3e; %d ids checked to 1e-6" % (worst, anchored))
    assert anchored >= 50
    ctx.close()


def test_player_cov_out_on_the_product_build(seq, tmp_path):
    from xrslam_amd.harness import euroc
    root = euroc.write_euroc(seq, str(tmp_path / "mav0"))
    out = tmp_path / "cov.txt"
    p = subprocess.run([PLAYER, "--slam", ly.BENCH_YAML, "--device", ly.SENSOR_320, "--euroc", str(root), "--bootstrap-frames", str(N),
                        "--no-undistort", "--cov-out", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [ln.split() for ln in out.read_text().splitlines()]
    assert len(rows) >= 15 and all(len(f) == 23 for f in rows)
    answered = [f for f in rows if int(f[22]) == 0]
    assert len(answered) >= 10 and all(int(f[22]) in (-1, 0) for f in rows)
    ts = [float(f[0]) for f in answered]
    assert ts == sorted(ts) and len(set(ts)) >= 3
    for f in answered:
        m = np.zeros((6, 6))
        m[np.triu_indices(6)] = [float(v) for v in f[1:22]]
        m = m + np.triu(m, 1).T
        assert np.all(np.isfinite(m)) and np.all(np.linalg.eigvalsh(m) > 0)


def test_grouped_member_equals_its_solo_run(seq, on_run):
    from xrslam_amd import _lib
    g = runner.Group(_lib.LIB_PATH)
    try:
        r = _run(seq, True, group=g)
    finally:
        g.close()
    assert r["log"] == on_run["log"] and len(r["seen"]) == len(on_run["seen"])
    for a, b in zip(r["seen"], on_run["seen"]):
        assert a[1] == b[1] and a[2] == b[2] and a[5] == b[5]
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[7], b[7]) and np.array_equal(a[8], b[8]) and a[9] == b[9]
