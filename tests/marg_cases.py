"""Marginalisation problems shared by the CPU measurement (tests/test_oracle_ba.py) and the GPU parity tests
(tests/test_marg_shapes_gpu.py): the shapes xrhip_ba_marginalize accepts and the pipeline builds, which the frame-0 chain of
tests/test_ba_gpu.py does not reach -- a victim that is not frame 0, a prior over a strict subset of the window, no landmarks, no
prior, a victim no landmark ties to the rest.  Every builder takes `marg(md) -> (sqrt_info, infovec, lin)` for the marginalisations a
case is chained on, so that the CPU tests chain on the oracle and the GPU tests on the device's own result, as the pipeline does."""
import numpy as np

from tests import ba_synth as bs
from xrslam_amd import abi


def marg_problem(pd, victim=0):
    """what Map::marginalize_frame assembles for `victim`: the prior, the IMU factors that touch the victim, and every observation of
    the landmarks the victim sees (as reference or as target)"""
    seen = set(pd.obs_lm[(pd.obs_ref == victim) | (pd.obs_tgt == victim)])
    sel = np.array([l in seen for l in pd.obs_lm], bool)
    obs = dict(tgt=pd.obs_tgt[sel], ref=pd.obs_ref[sel], lm=pd.obs_lm[sel], z_tgt=pd.obs_z_tgt[sel], z_ref=pd.obs_z_ref[sel])
    ki = np.where((pd.imu_i == victim) | (pd.imu_j == victim))[0]
    imu = dict(i=pd.imu_i[ki], j=pd.imu_j[ki], data=pd.imu_data[ki])
    prior = dict(frames=pd.prior_frames, sqrt_info=pd.prior_sqrt_info, infovec=pd.prior_infovec, lin=pd.prior_lin)
    return abi.MargProblemData(pd.frame_state, victim, pd.cam_ext, pd.imu_ext, pd.sqrt_inv_cov, prior, imu, pd.inv_depth, obs)


def next_window(pd, victim, si, iv, lin):
    """the window after marginalising `victim` of `pd`: the frame gone with its observations and the IMU factors that touched it,
    the prior (si, iv, lin) on the frames that remain"""
    K = len(pd.frame_state)
    rest = np.array([f for f in range(K) if f != victim])
    new = -np.ones(K, int)
    new[rest] = np.arange(K - 1)
    keep = (pd.obs_tgt != victim) & (pd.obs_ref != victim)
    obs = dict(tgt=new[pd.obs_tgt[keep]], ref=new[pd.obs_ref[keep]], lm=pd.obs_lm[keep], z_tgt=pd.obs_z_tgt[keep],
               z_ref=pd.obs_z_ref[keep])
    ki = (pd.imu_i != victim) & (pd.imu_j != victim)
    imu = dict(i=new[pd.imu_i[ki]], j=new[pd.imu_j[ki]], data=pd.imu_data[ki])
    prior = dict(frames=np.arange(K - 1), sqrt_info=si, infovec=iv, lin=lin)
    return abi.BaProblemData(pd.frame_state[rest], pd.frame_fix[rest], pd.cam_ext, pd.imu_ext, pd.sqrt_inv_cov, pd.inv_depth, None,
                             obs=obs, imu=imu, prior=prior)


def first_window(K=6, L=80, seed=22, **kw):
    """the window of tests/test_ba_gpu.py::test_marginalization_parity: moved off the prior's linearisation point"""
    pd, _ = bs.make_window(K=K, L=L, seed=seed, **kw)
    pd.frame_state[1:, 4:7] += 1e-3
    return pd


def chained_window(marg, K=6, L=80, seed=22, n=1):
    """the window that follows `n` frame-0 marginalisations: the prior is dense and the 1e15 gauge rows are gone.  (After one, the
    prior still carries the first marginalisation's rank deficiency; at K = 11, seed 21 it takes three before a victim in the middle
    leaves a positive definite marginal, i.e. before the Cholesky fast path can stand.)"""
    pd = first_window(K, L, seed)
    for _ in range(n):
        pd = next_window(pd, 0, *marg(marg_problem(pd, 0)))
    return pd


def subset_prior_window(marg, seed=22):
    """The pipeline's shape: the prior covers the frames that were in the window at the previous marginalisation, the keyframes that
    came since have no prior rows.  Frames, observations and IMU factors are those of frames 1 .. 7 of a K = 8 window; the prior is
    the frame-0 marginalisation of the K = 6 window of the same seed and trajectory (its five frames are this window's first five,
    linearised a few millimetres from where this window holds them)."""
    si, iv, lin = marg(marg_problem(first_window(6, 80, seed), 0))
    p8 = first_window(8, 80, seed)
    w = next_window(p8, 0, np.zeros((105, 105)), np.zeros(105), p8.frame_state[1:])
    w._set_prior(dict(frames=np.arange(5), sqrt_info=si, infovec=iv, lin=lin))
    return w


def without_landmarks(md):
    """only the IMU factors and the prior: n_landmarks = 0, n_obs = 0"""
    prior = dict(frames=md.prior_frames, sqrt_info=md.prior_sqrt_info, infovec=md.prior_infovec, lin=md.prior_lin)
    imu = dict(i=md.imu_i, j=md.imu_j, data=md.imu_data)
    return abi.MargProblemData(md.frame_state, md.victim, md.cam_ext, md.imu_ext, md.sqrt_inv_cov, prior, imu, np.zeros(0), None)


def unobserved_victim(pd, victim):
    """`pd` with every observation on the victim removed: only IMU factors and the prior tie the victim to the rest.  (The landmark
    array stays: the marginalisation then has landmarks and no observation of them.)"""
    out = pd.copy()
    keep = (pd.obs_tgt != victim) & (pd.obs_ref != victim)
    out._set_obs(dict(tgt=pd.obs_tgt[keep], ref=pd.obs_ref[keep], lm=pd.obs_lm[keep], z_tgt=pd.obs_z_tgt[keep],
                      z_ref=pd.obs_z_ref[keep]))
    return out


def has_foreign_reference(md):
    """does the victim see a landmark as a TARGET, with the reference elsewhere in the window?"""
    return bool(np.any((md.obs_tgt == md.victim) & (md.obs_ref != md.victim)))


# name -> (family of tests/marg_metric.py, builder(marg) -> MargProblemData).  K = 6, L = 80 (R = 75) has every block; K = 11, L = 150
# is the size at which the chained marginalisation reaches the Cholesky fast path.
def _c(family, fn):
    return family, fn


CASES = {
    # 1. the victim in the middle and last (one IMU factor); first window: make_window's 1e15 gauge rows on frame 0 stay in the result
    "first_v2": _c("gauge", lambda marg: marg_problem(first_window(), 2)),
    "first_vlast": _c("gauge", lambda marg: marg_problem(first_window(), 5)),
    "chained_v2": _c("chained", lambda marg: marg_problem(chained_window(marg), 2)),
    "chained_vlast": _c("chained", lambda marg: marg_problem(chained_window(marg), 4)),
    "chained_k11_v2": _c("chained", lambda marg: marg_problem(chained_window(marg, 11, 150, 21), 2)),
    "chained_k11_vlast": _c("chained", lambda marg: marg_problem(chained_window(marg, 11, 150, 21), 9)),
    "chained3_k11_v2": _c("chained", lambda marg: marg_problem(chained_window(marg, 11, 150, 21, n=3), 2)),
    # 2. the prior over five of seven frames
    "subset_prior": _c("chained", lambda marg: marg_problem(subset_prior_window(marg), 0)),
    # 3. no landmarks: a first (rank-deficient) marginalisation and a chained one
    "no_landmarks_first": _c("first", lambda marg: without_landmarks(marg_problem(first_window(), 0))),
    "no_landmarks_chained": _c("chained", lambda marg: without_landmarks(marg_problem(chained_window(marg), 0))),
    # 4. no prior
    "no_prior": _c("first", lambda marg: marg_problem(first_window(with_prior=False), 0)),
    # 5. a victim that no landmark connects to the rest
    "unobserved_first_v2": _c("gauge", lambda marg: marg_problem(unobserved_victim(first_window(), 2), 2)),
    "unobserved_chained_v0": _c("chained", lambda marg: marg_problem(unobserved_victim(chained_window(marg), 0), 0)),
}
