"""GPU: xrhip_ba_covariance (kc_compact, kc_factor, kc_selected_inverse, kc_landmark_var) against the inverse of the oracle's dense
normal equations.  Reference, metric and the per-case tolerance max(1e-9, 50 d_ref): tests/cov_model.py (profiles/covariance.md has
the table)."""
import numpy as np
import pytest

from tests import cov_model as cm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from xrslam_amd import ba
    c = ba.BaContext()
    yield c
    c.close()


def _check_blocks(name, blocks, sel):
    ref, (tol, _) = cm.reference(name), cm.tolerance(name)
    err = cm.block_error(blocks, ref["blocks"][sel])
    print("%s: block error max %.3e (tolerance %.3e, d_ref %.3e)" % (name, err.max(), tol, ref["d_blocks"].max()))
    assert err.max() <= tol
    for b in blocks:
        assert np.abs(b - b.T).max() <= 1e-14 * np.abs(b).max()


@pytest.mark.parametrize("name", cm.CASES)
def test_blocks_match_reference(ctx, name):
    """Every frame's 15 x 15 block: relative Frobenius error within the case's tolerance, symmetric to 1e-14, a positive diagonal on the
    free dofs and exact zeros on the constant ones; the problem's arrays come back unchanged."""
    pd = cm.problem(name).copy()
    before = (pd.frame_state.copy(), pd.inv_depth.copy())
    F = len(pd.frame_state)
    out = ctx.covariance(pd, np.arange(F))
    assert out["status"] == 0 and 0 < out["rcond"] <= 1
    assert np.array_equal(pd.frame_state, before[0]) and np.array_equal(pd.inv_depth, before[1])
    _check_blocks(name, out["blocks"], np.arange(F))
    for f in range(F):
        free = np.concatenate([np.full(6, not (pd.frame_fix[f] & 1)), np.full(9, not (pd.frame_fix[f] & 2))])
        b = out["blocks"][f]
        assert np.all(np.diag(b)[free] > 0)
        assert np.all(b[~free] == 0) and np.all(b[:, ~free] == 0)


@pytest.mark.parametrize("name", ("k6", "k36_l40", "s1_window"))
def test_selection(ctx, name):
    """One frame, all frames, a repeated index: the blocks of "all" equal the blocks of one-at-a-time bit for bit."""
    pd = cm.problem(name).copy()
    F = len(pd.frame_state)
    every = ctx.covariance(pd, np.arange(F))["blocks"]
    for f in (0, F // 2, F - 1):
        one = ctx.covariance(pd, [f])
        assert one["status"] == 0 and np.array_equal(one["blocks"][0], every[f])
    rep = ctx.covariance(pd, [F - 1, 1, F - 1])["blocks"]
    assert np.array_equal(rep[0], every[F - 1]) and np.array_equal(rep[1], every[1]) and np.array_equal(rep[2], every[F - 1])
    many = np.arange(150) % F   # more than one launch of kc_selected_inverse (64 selected frames each)
    assert np.array_equal(ctx.covariance(pd, many)["blocks"], every[many])


def test_schur_study_mode_does_not_reach_the_covariance(ctx):
    """A context left in the bf16 study mode of the Schur contraction (xrhip_ba_debug_set_schur_precision) still computes the
    covariance's Schur product in f64: the same bits as before."""
    pd = cm.problem("k11").copy()
    want = ctx.covariance(pd, [10], landmarks=True)
    ctx.set_schur_precision(2)
    try:
        got = ctx.covariance(pd, [10], landmarks=True)
    finally:
        ctx.set_schur_precision(0)
    assert got["status"] == 0 and np.array_equal(got["blocks"], want["blocks"]) and np.array_equal(got["var"], want["var"])


def test_fix_motion_frame_has_zero_rows(ctx):
    from xrslam_amd import abi
    pd = cm.problem("k6").copy()
    pd.frame_fix[2] = abi.FIX_MOTION
    out = ctx.covariance(pd, [2, 3], landmarks=True)
    assert out["status"] == 0
    b = out["blocks"][0]
    assert np.all(b[6:] == 0) and np.all(b[:, 6:] == 0) and np.all(np.diag(b)[:6] > 0)
    assert np.all(np.diag(out["blocks"][1]) > 0)


@pytest.mark.parametrize("name", cm.LANDMARK_CASES)
def test_landmark_variances(ctx, name):
    """kc_landmark_var: relative error per variance within the case's tolerance; a constant landmark has variance 0; the blocks of the
    full-inverse path hold the same tolerance as those of the direct one."""
    pd = cm.problem(name).copy()
    F = len(pd.frame_state)
    ref, (_, tol) = cm.reference(name), cm.tolerance(name)
    out = ctx.covariance(pd, np.arange(F), landmarks=True)
    assert out["status"] == 0
    err = cm.var_error(out["var"], ref["var"])
    print("%s: variance error max %.3e (tolerance %.3e)" % (name, err.max(), tol))
    assert err.max() <= tol
    assert np.all(out["var"][ref["var"] > 0] > 0) and np.all(out["var"][ref["var"] == 0] == 0)
    _check_blocks(name, out["blocks"], np.arange(F))


def test_fixed_landmark_has_zero_variance(ctx):
    pd = cm.problem("k11").copy()
    pd.landmark_fix[[0, 7, 149]] = 1
    out = ctx.covariance(pd, [10], landmarks=True)
    assert out["status"] == 0
    assert np.all(out["var"][[0, 7, 149]] == 0) and np.count_nonzero(out["var"]) >= 140


def test_localize_all_landmarks_constant_launches_no_variance_kernel(ctx):
    """make_localize: one free frame, every landmark constant -- variances exactly 0, and the call with variances launches exactly what
    the call without them does (no full inverse, no kc_landmark_var)."""
    pd = cm.problem("localize").copy()
    ctx.stats(reset=True)
    a = ctx.covariance(pd, [3])
    n_a = ctx.stats(reset=True).n_cov_launches
    b = ctx.covariance(pd, [3], landmarks=True)
    n_b = ctx.stats(reset=True).n_cov_launches
    assert a["status"] == 0 and b["status"] == 0 and n_a > 0 and n_a == n_b
    assert np.all(b["var"] == 0) and np.array_equal(a["blocks"], b["blocks"])
    _check_blocks("localize", a["blocks"], np.array([3]))


def test_rank_deficient_window_is_reported(ctx):
    """No prior, nothing fixed: the gauge is free.  Status 1, outputs as pre-filled, return code 0 -- and the context then solves
    s1_localize with the summary the fixture records."""
    from tests import ba_snapshots, ba_synth as bs
    pd = bs.make_window(K=6, L=40, seed=5, with_prior=False)[0]
    out = ctx.covariance(pd, [0, 5], landmarks=True, prefill=-7.0)
    assert out["status"] == 1 and out["rcond"] == 0
    assert np.all(out["blocks"] == -7.0) and np.all(out["var"] == -7.0)
    name, loc, exp = [s for s in ba_snapshots.load_all() if s[0] == "s1_localize"][0]
    sm = ctx.solve(loc)
    assert sm.iterations == int(exp["iterations"]) and sm.termination == int(exp["termination"])
    assert abs(sm.final_cost - float(exp["final_cost"])) <= 1e-8 * float(exp["final_cost"])


def test_argument_errors(ctx):
    import ctypes as C

    from tests import ba_synth as bs
    from xrslam_amd import _lib
    pd = cm.problem("k6").copy()
    with pytest.raises(RuntimeError, match="out of range"):
        ctx.covariance(pd, [6])
    with pytest.raises(RuntimeError, match="out of range"):
        ctx.covariance(pd, [-1])
    lib = ctx._lib
    s = pd.struct()
    assert lib.xrhip_ba_covariance(ctx._h, C.byref(s), None) == _lib.XRHIP_EINVAL
    big = bs.make_window(K=65, L=10, seed=2)[0]   # 975 free dofs: over the cap of 960
    with pytest.raises(RuntimeError, match="960"):
        ctx.covariance(big, [0])
    ok = ctx.covariance(pd, [5])
    assert ok["status"] == 0 and np.array_equal(ok["blocks"][0], ctx.covariance(pd, np.arange(6))["blocks"][5])
