"""GPU: xrhip_ba_covariance (kc_compact, kc_factor, kc_selected_inverse, kc_landmark_var) against the inverse of the oracle's dense
normal equations.  Reference, metric and the per-case tolerance max(1e-9, 50 d_ref): tests/cov_model.py (profiles/covariance.md has
the table).  The cases run to the cap (na = 960 = n16: 60 tile columns in kc_factor, 60 workgroups of the full inverse); the partly
constant frames, the landmark edges, rcond and the ill-conditioned family are measured against the 50-digit reference
(cov_model.reference_hp)."""
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


def _check_blocks(name, blocks, sel, hp=False):
    ref, (tol, _) = cm.reference_hp(name) if hp else cm.reference(name), cm.tolerance(name)
    err = cm.block_error(blocks, ref["blocks"][sel])
    print("%s: block error max %.3e (tolerance %.3e, d_ref %.3e%s)" % (name, err.max(), tol, cm.reference(name)["d_blocks"].max(),
                                                                      ", against 50 digits" if hp else ""))
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
    _check_zeros(pd, out["blocks"])


def _check_zeros(pd, blocks):
    """a positive diagonal on the free dofs, exact zeros in the rows and columns of the constant ones"""
    for f in range(len(pd.frame_state)):
        free = np.concatenate([np.full(6, not (pd.frame_fix[f] & 1)), np.full(9, not (pd.frame_fix[f] & 2))])
        b = blocks[f]
        assert np.all(np.diag(b)[free] > 0)
        assert np.all(b[~free] == 0) and np.all(b[:, ~free] == 0)


def test_cap_in_three_launches(ctx):
    """na = 960 = n16 (no identity tail), 150 selected frames: three launches of kc_selected_inverse that reuse the 64 right-hand-side
    slots -- every block within the tolerance, and the bits of the one-launch call."""
    pd = cm.problem("k64").copy()
    every = ctx.covariance(pd, np.arange(64))
    many = np.arange(150) % 64
    out = ctx.covariance(pd, many)
    assert every["status"] == 0 and out["status"] == 0 and out["rcond"] == every["rcond"]
    _check_blocks("k64", out["blocks"], many)
    assert np.array_equal(out["blocks"], every["blocks"][many])


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


def test_scratch_that_moves_between_requests():
    """One context of its own: k6 (na = 90: 0.17 MiB of scratch, the 1 MiB floor), k21 (na = 315: 1.7 MiB, so the block is reallocated
    behind a drained stream and every buffer moves), k6 again in the larger block -- every frame's block within the case's tolerance."""
    from tests.test_ba_stage_host import COV_SCRATCH, cov_args, scratch_expected
    from xrslam_amd import ba
    need = {name: scratch_expected(COV_SCRATCH, *cov_args(15 * K, K, False, len(cm.problem(name).inv_depth)))[1]
            for name, K in (("k6", 6), ("k21", 21))}
    assert need["k6"] <= 1 << 20 < need["k21"]
    c = ba.BaContext()
    try:
        for name in ("k6", "k21", "k6"):
            pd = cm.problem(name).copy()
            F = len(pd.frame_state)
            assert cm.reference(name)["na"] == 15 * F
            out = c.covariance(pd, np.arange(F))
            assert out["status"] == 0
            _check_blocks(name, out["blocks"], np.arange(F))
            _check_zeros(pd, out["blocks"])
    finally:
        c.close()


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
    _check_zeros(pd, out["blocks"])
    # one selected frame: the full inverse still runs one workgroup per tile column, each with right-hand-side scratch of its own
    one = ctx.covariance(pd, [F - 1], landmarks=True)
    assert one["status"] == 0 and np.array_equal(one["var"], out["var"]) and np.array_equal(one["blocks"][0], out["blocks"][F - 1])


@pytest.mark.parametrize("landmarks", (False, True), ids=("direct", "full"))
@pytest.mark.parametrize("name", cm.PARTIAL_CASES)
def test_partly_constant_frames(ctx, name, landmarks):
    """FIX_POSE or FIX_MOTION alone (-1 slots inside a frame's 16-column group, which in k5_straddle lies across a tile boundary): the
    blocks and variances against the 50-digit reference within the case's tolerance, constant rows and columns exactly 0, and every
    partly constant frame asked for alone gives the bits it has among all."""
    pd = cm.problem(name).copy()
    F = len(pd.frame_state)
    hp, (_, tol_v) = cm.reference_hp(name), cm.tolerance(name)
    out = ctx.covariance(pd, np.arange(F), landmarks=landmarks)
    assert out["status"] == 0
    _check_blocks(name, out["blocks"], np.arange(F), hp=True)
    _check_zeros(pd, out["blocks"])
    if landmarks:
        err = cm.var_error(out["var"], hp["var"])
        print("%s: variance error max %.3e (tolerance %.3e, against 50 digits)" % (name, err.max(), tol_v))
        assert err.max() <= tol_v
        assert np.array_equal(out["var"] == 0, hp["var"] == 0) and np.all(out["var"] >= 0)
    partial = [f for f in range(F) if pd.frame_fix[f] in (1, 2)]
    assert partial
    for f in partial + [F - 1]:
        one = ctx.covariance(pd, [f], landmarks=landmarks)
        assert one["status"] == 0 and np.array_equal(one["blocks"][0], out["blocks"][f])
        if landmarks:
            assert np.array_equal(one["var"], out["var"])


@pytest.mark.parametrize("name", cm.EDGE_CASES)
def test_landmark_edges(ctx, name):
    """kc_landmark_var at its edges, full path: a last group of one, two and three landmarks ending in a free one, a constant landmark
    next to free ones in it, and a landmark seen only by constant frames -- its row of W has no free entry, so its variance is 1 / hll
    of the oracle's H to 1e-14.  Everything else against the 50-digit reference within the case's tolerance."""
    pd = cm.problem(name).copy()
    F, L = len(pd.frame_state), len(pd.inv_depth)
    ref, hp, (_, tol_v) = cm.reference(name), cm.reference_hp(name), cm.tolerance(name)
    out = ctx.covariance(pd, np.arange(F), landmarks=True)
    assert out["status"] == 0 and len(out["var"]) == L
    err = cm.var_error(out["var"], hp["var"])
    print("%s: variance error max %.3e (tolerance %.3e, against 50 digits)" % (name, err.max(), tol_v))
    assert err.max() <= tol_v
    assert np.array_equal(out["var"] == 0, hp["var"] == 0) and np.array_equal(out["var"] == 0, pd.landmark_fix != 0)
    lone = cm.EDGE_LONELY
    assert abs(out["var"][lone] * ref["hll"][lone] - 1.0) <= 1e-14
    assert out["var"][L - 1] > 1.0 / ref["hll"][L - 1]
    _check_blocks(name, out["blocks"], np.arange(F), hp=True)
    _check_zeros(pd, out["blocks"])


@pytest.mark.parametrize("name", [n for n in cm.HP_CASES if n not in cm.ILL_CASES] + list(cm.LARGE_CASES))
def test_rcond_is_the_pivot_ratio(ctx, name):
    """rcond = min pivot / max pivot of the Jacobi-scaled factor.  Small cases: against the 50-digit pivot ratio, within 50 times
    the relative error of numpy's own pivot ratio against it, plus 1e-12.  Large cases: against numpy's pivot ratio at 1e-6."""
    pd = cm.problem(name).copy()
    out = ctx.covariance(pd, [len(pd.frame_state) - 1])
    assert out["status"] == 0
    r = cm.reference(name)
    want = cm.reference_hp(name)["rcond"] if name in cm.HP_CASES else r["piv_min"] / r["piv_max"]
    tol = cm.rcond_tolerance(name)
    err = abs(out["rcond"] - want) / want
    print("%s: rcond %.9e, reference %.9e, relative error %.3e (tolerance %.3e)" % (name, out["rcond"], want, err, tol))
    assert err <= tol


@pytest.mark.parametrize("name", cm.ILL_CASES)
def test_ill_conditioned_family(ctx, name):
    """One window behind a progressively weaker gauge prior, cond(scaled S) 5e8 ... 1e14.  Where numpy factors the scaled S with min
    pivot > 100 na 2^-52 max pivot the device answers (status 0); where it answers, the largest block and variance error against the
    50-digit reference is within 50 times the numpy route's own largest error against it, plus 1e-12, on both paths, and rcond is the
    50-digit pivot ratio within 50 times numpy's own error; where it does not, the outputs are as pre-filled."""
    pd = cm.problem(name).copy()
    F = len(pd.frame_state)
    hp = cm.reference_hp(name)
    assert hp["pd"]   # (tests/test_cov_model.py: every member is positive definite at 50 digits -- none is left unmeasured)
    tol_b, tol_v = cm.tolerance_hp(name)
    for landmarks in (False, True):
        out = ctx.covariance(pd, np.arange(F), landmarks=landmarks, prefill=-7.0)
        print("%s (%s): status %d, rcond %.6e (50 digits %.6e)" % (name, "full" if landmarks else "direct", out["status"], out["rcond"], hp["rcond"]))
        if cm.factorable(name):
            assert out["status"] == 0
        if out["status"] != 0:
            assert out["status"] == 1 and out["rcond"] == 0 and np.all(out["blocks"] == -7.0)
            continue
        eb = cm.block_error(out["blocks"], hp["blocks"]).max()
        print("%s (%s): block error max %.3e (tolerance %.3e, numpy route %.3e)" % (name, "full" if landmarks else "direct", eb, tol_b, hp["err2_blocks"]))
        assert eb <= tol_b
        assert abs(out["rcond"] - hp["rcond"]) / hp["rcond"] <= cm.rcond_tolerance(name)
        if landmarks:
            ev = cm.var_error(out["var"], hp["var"]).max()
            print("%s: variance error max %.3e (tolerance %.3e, numpy route %.3e)" % (name, ev, tol_v, hp["err2_var"]))
            assert ev <= tol_v


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


def test_all_frames_constant_is_status_two(ctx):
    """No free frame dof: status 2, rcond 0, outputs as pre-filled, return code 0 (nothing is launched)."""
    pd = cm.problem("k6").copy()
    pd.frame_fix[:] = 3
    ctx.stats(reset=True)
    out = ctx.covariance(pd, [0, 5], landmarks=True, prefill=-7.0)
    assert out["status"] == 2 and out["rcond"] == 0 and ctx.stats(reset=True).n_cov_launches == 0
    assert np.all(out["blocks"] == -7.0) and np.all(out["var"] == -7.0)


def test_free_frame_without_factors_is_reported(ctx):
    """A free last frame touched by no observation, IMU factor or prior row: its diagonal of S is 0, kc_compact leaves A_ii = 0 and the
    first of its pivots fails.  Status 1, outputs as pre-filled, return code 0 -- and the context then solves s1_localize as recorded."""
    from tests import ba_snapshots
    pd = cm.unanchored_last_frame()
    for landmarks in (False, True):
        out = ctx.covariance(pd, [0, 5], landmarks=landmarks, prefill=-7.0)
        assert out["status"] == 1 and out["rcond"] == 0
        assert np.all(out["blocks"] == -7.0) and (not landmarks or np.all(out["var"] == -7.0))
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
