"""Hard bundle-adjustment problems for the termination tests: the shapes of the size routes (tests/test_ba_routes_gpu.py) pushed to where
the trust-region loop stops in every way it can -- far starts, gross outliers under the Cauchy loss, landmarks behind the camera, an
iteration limit of any value, a problem that starts at its minimum -- and `profile`, which reads off an oracle trace the facts a test
conditions on (so that a case cannot pass without the run of rejections it was written for).  A plain module: no fixtures."""
import numpy as np

from tests import ba_synth as bs
from xrslam_amd import abi

CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2

HELD = abi.FIX_POSE | abi.FIX_MOTION


def _free_prior(states, frames, seed):
    """A prior on `frames` linearised a little away from their states: diagonal sqrt-information (0.01 rad / 1 cm on the pose,
    0.1 m/s and the biases' random walk on the motion), infovec zero."""
    rng = np.random.RandomState(seed)
    n = 15 * len(frames)
    w = np.tile(np.concatenate([np.full(6, 100.0), np.full(3, 10.0), np.full(3, 1e3), np.full(3, 1e2)]), len(frames))
    lin = states[frames].copy()
    lin[:, 4:7] += 1e-3 * rng.randn(len(frames), 3)
    return dict(frames=np.asarray(frames), sqrt_info=np.diag(w), infovec=np.zeros(n), lin=lin)


def window(K, L, seed, prior, fixed=0, noise=1.0):
    """refine_window-shaped: free landmarks (a Schur complement), all frames free but the first `fixed`; with the window's gauge
    prior (ba_synth.make_window) or without a prior.  na = 15 (K - fixed).  noise: ba_synth's state_noise, the distance of the start
    from the truth in units of 2 mrad / 4 mm / 3 % of a depth."""
    return bs.make_window(K=K, L=L, seed=seed, with_prior=prior, n_fixed_first=fixed, state_noise=noise)[0]


def one_free(K, L, seed, prior, all_imu=False, j=None):
    """localize_newframe-shaped: only the last frame free, every landmark held, the reprojection factors into the last frame.
    all_imu: keep all K - 1 IMU factors (NI > 8 rules out kb_chain without a prior).  na = 15.
    j: free frame j instead of the last, with the IMU factors on both sides of it -- the free frame then is the one a factor reads its
    bias linearisation point from, which moves with every accepted step (tests/tr_model.py): the source of the rejection runs."""
    pd, truth = bs.make_window(K=K, L=L, seed=seed, with_prior=False)
    j = K - 1 if j is None else j
    fix = np.full(K, HELD, np.uint8)
    fix[j] = 0
    keep = pd.obs_tgt == j
    obs = dict(tgt=pd.obs_tgt[keep], ref=pd.obs_ref[keep], lm=pd.obs_lm[keep], z_tgt=pd.obs_z_tgt[keep], z_ref=pd.obs_z_ref[keep])
    states = truth["states"].copy()
    states[j] = pd.frame_state[j]
    ki = np.arange(len(pd.imu_j)) if all_imu else np.where((pd.imu_j == j) | (pd.imu_i == j))[0]
    imu = dict(i=pd.imu_i[ki], j=pd.imu_j[ki], data=pd.imu_data[ki])
    pr = _free_prior(states, [j], seed) if prior else None
    return abi.BaProblemData(states, fix, bs.CAM_EXT, bs.IMU_EXT, bs.SQRT_INV_COV, truth["inv_depth"], np.ones(L, np.uint8),
                             obs=obs, imu=imu, prior=pr, max_iterations=30)


def subwindow(K, L, seed, prior, first_imu=True):
    """refine_subwindow-shaped: frame 0 held, frames 1 .. K-1 free, every landmark held, only the reprojection factors of the
    landmarks frame 0 anchors (no factor between two free poses).  first_imu=False drops the IMU factor 0 -> 1.  na = 15 (K - 1)."""
    pd, _ = bs.make_window(K=K, L=L, seed=seed, with_prior=False, n_fixed_first=1)
    keep = pd.obs_ref == 0
    obs = dict(tgt=pd.obs_tgt[keep], ref=pd.obs_ref[keep], lm=pd.obs_lm[keep], z_tgt=pd.obs_z_tgt[keep], z_ref=pd.obs_z_ref[keep])
    ki = (pd.imu_i >= 0) if first_imu else (pd.imu_i > 0)
    imu = dict(i=pd.imu_i[ki], j=pd.imu_j[ki], data=pd.imu_data[ki])
    pr = _free_prior(pd.frame_state, list(range(1, K)), seed) if prior else None
    return abi.BaProblemData(pd.frame_state, pd.frame_fix, bs.CAM_EXT, bs.IMU_EXT, bs.SQRT_INV_COV, pd.inv_depth,
                             np.ones(L, np.uint8), obs=obs, imu=imu, prior=pr, max_iterations=30)


def dims(pd):
    """The sizes the route decisions read: M (reprojection factors), NI, NP, na, F."""
    free = [(f & abi.FIX_POSE) == 0 for f in pd.frame_fix], [(f & abi.FIX_MOTION) == 0 for f in pd.frame_fix]
    na = 6 * sum(free[0]) + 9 * sum(free[1])
    return dict(M=len(pd.obs_tgt), NI=len(pd.imu_i), NP=len(pd.prior_frames), na=na, F=len(pd.frame_state))


def route(kind, use_lds=2, block=512, wt=0, wf=0):
    """What xrhip_ba_debug_last_route should report (na and F are checked against the problem)."""
    multi = kind in ("small_mid", "multi")
    return dict(route=kind, use_lds=-1 if kind == "chain" else use_lds, sred_tiled=int(multi and use_lds == 0),
                block=block if multi else 0, wide_trials=wt, wide_first=wf)


# ------------------------------------------------------------------------------------------------ hard starts
def free_frames(pd):
    return [f for f in range(len(pd.frame_state)) if (int(pd.frame_fix[f]) & 3) != 3]


def with_max_iterations(pd, m):
    pd = pd.copy()
    pd.max_iterations = int(m)
    return pd


def far(pd, dp=0.3, dv=1.0, rot=0.0, seed=0, max_iterations=None):
    """The free frames moved away from where the builder left them: every position by +dp m and every velocity by +dv m/s on each
    axis, every attitude by a rotation of `rot` rad about a seeded random axis."""
    pd = pd.copy()
    rng = np.random.RandomState(seed)
    for f in free_frames(pd):
        pd.frame_state[f, 4:7] += dp
        pd.frame_state[f, 7:10] += dv
        if rot:
            ax = rng.randn(3)
            pd.frame_state[f, 0:4] = bs.qmul(pd.frame_state[f, 0:4], bs.qexp(rot * ax / np.linalg.norm(ax)))
    if max_iterations is not None:
        pd.max_iterations = int(max_iterations)
    return pd


def outliers(pd, frac, px, seed, max_iterations=None):
    """A fraction `frac` of the reprojection observations (seeded choice) moved by `px` pixels in a random direction: gross
    mismatches, whose squared residual s = |r|^2 sits far out on the Cauchy loss (rho' = 1 / (1 + s))."""
    pd = pd.copy()
    rng = np.random.RandomState(seed)
    M = len(pd.obs_tgt)
    pick = rng.choice(M, int(round(frac * M)), replace=False)
    fx, fy = bs.K_EUROC[0], bs.K_EUROC[1]
    for o in pick:
        z = pd.obs_z_tgt[o]
        a = rng.uniform(0, 2 * np.pi)
        u = np.array([z[0] / z[2] + px * np.cos(a) / fx, z[1] / z[2] + px * np.sin(a) / fy, 1.0])
        pd.obs_z_tgt[o] = u / np.linalg.norm(u)
    if max_iterations is not None:
        pd.max_iterations = int(max_iterations)
    return pd


def flip_depths(pd, every=7):
    """Every `every`-th landmark behind its reference camera (negative inverse depth)."""
    pd = pd.copy()
    pd.inv_depth[::every] *= -1.0
    return pd


def prior_only(n_free=1, seed=1):
    """Nothing but a prior on the last `n_free` frames, linearised at their states, infovec zero: the cost and the gradient are zero
    at the start, the minimiser stops by the gradient test before its first iteration."""
    pd, _ = bs.make_window(K=n_free + 1, L=8, seed=seed, with_prior=False, n_fixed_first=1)
    frames = list(range(1, n_free + 1))
    pr = _free_prior(pd.frame_state, frames, seed)
    pr["lin"] = pd.frame_state[frames].copy()
    return abi.BaProblemData(pd.frame_state, pd.frame_fix, bs.CAM_EXT, bs.IMU_EXT, bs.SQRT_INV_COV, pd.inv_depth,
                             np.ones(len(pd.inv_depth), np.uint8), prior=pr, max_iterations=30)


def cauchy_s(pd):
    """Squared norm of every reprojection residual at pd's state: the argument of the Cauchy loss."""
    from oracle import ba_oracle as bo
    s = np.zeros(len(pd.obs_tgt))
    for o in range(len(s)):
        r = bo.eval_reprojection(pd.frame_state[pd.obs_tgt[o]], pd.frame_state[pd.obs_ref[o]], pd.inv_depth[pd.obs_lm[o]],
                                 pd.obs_z_tgt[o], pd.obs_z_ref[o], pd.cam_ext, pd.sqrt_inv_cov, jac=False)[0]
        s[o] = float(r @ r)
    return s


def saturated(pd, frac, px, seed, flip=False):
    """outliers() (and flip_depths()), with the guarantee the saturated-loss tests rest on: at least 20 observations start at s > 100."""
    pd = outliers(pd, frac, px, seed)
    if flip:
        pd = flip_depths(pd)
    assert int((cauchy_s(pd) > 100.0).sum()) >= 20
    return pd


# ------------------------------------------------------------------------------------------------ what a trace shows
def profile(trace, summary, pd=None):
    """The facts of an oracle solve (oracle.ba_oracle.solve_trace) the tests condition on.  trace rows: the trials that reached the
    accept / reject decision, column 8 = accepted.
      longest_run     the longest run of consecutive rejected trials
      trailing_run    rejected trials between the last accepted step (or the start) and the end of the solve
      limit_in_run    the iteration limit ended the solve, and the trial before it was a rejection (trailing_run deep in a run)
      termination, iterations, successes, usable   the summary's
      min_radius      the smallest trust-region radius a trial ran at
      saturated       (pd given) observations that start with a Cauchy argument s > 100"""
    acc = [bool(r[8]) for r in trace]
    longest = run = 0
    for a in acc:
        run = 0 if a else run + 1
        longest = max(longest, run)
    limit = summary.termination == NO_CONVERGENCE and len(acc) > 0 and int(trace[-1][0]) == summary.iterations
    out = dict(longest_run=longest, trailing_run=run, limit_in_run=bool(limit and run >= 1), termination=int(summary.termination),
               iterations=int(summary.iterations), successes=int(summary.successful_steps), usable=int(summary.usable),
               min_radius=float(min((r[5] for r in trace), default=np.inf)))
    if pd is not None:
        out["saturated"] = int((cauchy_s(pd) > 100.0).sum())
    return out


def limit_values(trace):
    """From the trace of a solve with a generous limit: (the smallest max_iterations >= 3 that ends the solve on a rejected trial,
    the smallest that ends it 3 trials deep in a run of rejections -- 2 deep if no run is longer), or None where the trace has none.
    A smaller limit replays the same trials and stops early, so the values hold for the limited solve -- which the caller asserts."""
    it = [int(r[0]) for r in trace]
    acc = [bool(r[8]) for r in trace]
    assert it == list(range(1, len(it) + 1)), "a trial did not reach its decision"
    depth, run = [], 0
    for a in acc:
        run = 0 if a else run + 1
        depth.append(run)
    ends = [i for i, d in zip(it, depth) if d >= 1 and i >= 3]
    deep = [i for i, d in zip(it, depth) if d == 3] or [i for i, d in zip(it, depth) if d == 2]
    return (ends[0] if ends else None), (deep[0] if deep else None)


def check_profile(p, want, tag=""):
    """Asserts that a profile has what a case was written for.  want: iterations / successes / termination (exact), limit_in_run,
    trailing = (min, max) of trailing_run, longest_min.  (`reason` is tr_model's: the oracle does not report which test fired.)"""
    for k in ("iterations", "successes", "termination", "limit_in_run"):
        if k in want:
            assert p[k] == want[k], (tag, k, p, want)
    if "trailing" in want:
        assert want["trailing"][0] <= p["trailing_run"] <= want["trailing"][1], (tag, p, want)
    if "longest_min" in want:
        assert p["longest_run"] >= want["longest_min"], (tag, p, want)


def exact_radius(r):
    """True if r is 1e4 3^a / 2^k: the initial radius, halved by rejections and tripled by accepted steps of length `radius` -- the
    values a trust-region radius takes without an implementation's own |step| entering it."""
    x = float(r) / 1e4
    for _ in range(80):
        if x == int(x):
            break
        x *= 2.0
    n = int(x)
    if n != x or n < 1:
        return False
    while n % 2 == 0:
        n //= 2
    while n % 3 == 0:
        n //= 3
    return n == 1


def stationary(pd):
    """pd made a problem that STARTS at a stationary point with a cost above zero: the gradient test stops it before the first
    iteration.  The oracle solves pd (again and again, from its own result, until it takes no further step: the bias reference of
    the IMU factors moves with every solve).  With a prior, the prior is then re-linearised at that state with the infovec that
    cancels what is left of the other factors' gradient (the prior's Jacobian is its diagonal sqrt-information there), which takes
    the gradient down to the rounding of its own sums; without one the repeated solves must get there themselves."""
    from oracle import ba_oracle as bo
    pd = pd.copy()
    pd.max_iterations = 50
    for _ in range(12):
        if bo.solve(pd).iterations == 0:
            break
    if len(pd.prior_frames):
        bare = abi.BaProblemData(pd.frame_state, pd.frame_fix, pd.cam_ext, pd.imu_ext, pd.sqrt_inv_cov, pd.inv_depth, pd.landmark_fix,
                                 obs=dict(tgt=pd.obs_tgt, ref=pd.obs_ref, lm=pd.obs_lm, z_tgt=pd.obs_z_tgt, z_ref=pd.obs_z_ref),
                                 imu=dict(i=pd.imu_i, j=pd.imu_j, data=pd.imu_data))
        _, _, g, po, mo, _ = bo.linearize(bare)
        w = np.diag(pd.prior_sqrt_info)
        assert np.count_nonzero(pd.prior_sqrt_info) == len(w)
        iv = np.zeros(len(w))
        for i, f in enumerate(pd.prior_frames):
            if po[f] >= 0:
                iv[15 * i:15 * i + 6] = -g[po[f]:po[f] + 6] / w[15 * i:15 * i + 6]
            if mo[f] >= 0:
                iv[15 * i + 6:15 * i + 15] = -g[mo[f]:mo[f] + 9] / w[15 * i + 6:15 * i + 15]
        pd = abi.BaProblemData(pd.frame_state, pd.frame_fix, pd.cam_ext, pd.imu_ext, pd.sqrt_inv_cov, pd.inv_depth, pd.landmark_fix,
                               obs=dict(tgt=pd.obs_tgt, ref=pd.obs_ref, lm=pd.obs_lm, z_tgt=pd.obs_z_tgt, z_ref=pd.obs_z_ref),
                               imu=dict(i=pd.imu_i, j=pd.imu_j, data=pd.imu_data),
                               prior=dict(frames=pd.prior_frames, sqrt_info=pd.prior_sqrt_info, infovec=iv,
                                          lin=pd.frame_state[pd.prior_frames].copy()))
    pd.max_iterations = 30
    return pd


def gradient_max(pd):
    """Largest entry of the oracle's gradient at pd's state (the local coordinates are the ambient ones to first order)."""
    from oracle import ba_oracle as bo
    return float(np.abs(bo.linearize(pd)[2]).max())
