"""Oracle parity of xrhip_ba_solve on every way the trust-region loop stops, on every route that runs it.

tests/test_ba_routes_gpu.py holds every size route to the oracle on friendly problems: they converge by function tolerance or run out
of 30 iterations at the end of a long rejection tail.  The cases here take the same shapes (tests/ba_hard.py) to the other exits of
the loop (ba_kernels.hip.h: trial_begin, trial_decide; ba_chain.hip.h):

  m0 / m1 / m2   max_iterations = 0, 1, 2
  mrej           the smallest limit >= 3 that ends the solve on a rejected trial
  mdeep          a limit that strikes three trials deep in a run of rejections (two where no run is longer): the `k > 0` replay at the
                 top of trial_decide -- inside one batch of try_block, and inside one kb_trials_wide launch on the wide routes (the
                 run's 2nd .. 8th trial are never the first of a launch)
  m200           the same start with max_iterations = 200: the run of ~30 rejections halves the radius until the step is below the
                 parameter tolerance -- CONVERGENCE out of a rejection run (tests/test_ba_termination_model.py pins that it is the
                 parameter test that fires)
  grad0          a prior-only problem at its minimum: the gradient test at iteration 0

mrej and mdeep are derived from the oracle's trace of the m200 problem as the module is collected; every case then asserts on the
oracle's trace of its OWN problem that it has the property it is named for (`want`, ba_hard.check_profile), asserts the route the
device took (xrhip_ba_debug_last_route), and holds the device to the oracle with tests/ba_parity.solve_both: iterations, accepted
steps, termination and usable exactly, states to rtol 1e-7, costs to 1e-9 / 1e-8.

The rejection runs come from the reference's live bias reference (tests/tr_model.py): a free frame that some IMU factor STARTS at.
one_free(..., j=2) frees a middle frame for that reason -- with the last frame free, no start (translated, rotated by 0.2 - 0.5 rad,
30 % outliers) made kb_tiny / kb_small_mid reject a single trial.

The choice of cases.  tests/test_ba_termination_model.py holds the oracle to an independent model on every case of this table, radii
bit for bit.  Two double-precision solvers can agree on a radius bit for bit only while it is 1e4 3^a / 2^k: an accepted step with a
relative decrease above 0.75 sets it to 3 |step|, and unless the step is the scaled gradient of length `radius`, |step| comes out of
each implementation's own linear solve.  So the starts are those, among seeds 1 - 12 of each shape at 1, 0.3, 0.1 and 0.03 of far()'s
distance, on which the oracle's trace has a rejection run that ends in convergence and the oracle and the model agree on every radius
(the model test asserts it; on the two block-256 shapes that includes one radius of 3 |step| on which they agree to the bit); nothing
the device computes entered the choice.  refine_window-shaped problems
with the 1e15 gauge prior are in the table only at F = 33 (too slow for the model): started far out, oracle and model agree on every
decision but only to 7e-9 in the costs and 5e-9 in the states.  The windows of LANDMARKS (no gauge prior) reach a radius of 3 |step|
later in their solves, so only their limited solves are cases.

The second table holds the saturated Cauchy loss (gross outliers: s = |r|^2 > 100 on at least 20 observations) and landmarks behind
their camera, as solve parity and as linearisation parity.  The third pins the contract for non-finite input."""
import numpy as np
import pytest

from tests import ba_hard as bh
from tests.ba_hard import CONVERGENCE, NO_CONVERGENCE, dims, far, one_free, route, subwindow, window
from tests.ba_parity import compare_linearization, solve_both

pytestmark = pytest.mark.gpu

# id: (far-start problem, the route it must take).  Shapes at or below those of the routes test for the same route.
BASES = {
    "tiny": (lambda: far(one_free(4, 300, 3, True, j=2)), route("tiny")),
    "chain_one_free": (lambda: far(one_free(4, 300, 3, False, j=2)), route("chain")),
    "chain_free3": (lambda: far(subwindow(4, 60, 5, False)), route("chain")),
    "small_mid": (lambda: far(one_free(4, 780, 3, True, j=2)), route("small_mid", wt=1)),
    "multi_block256": (lambda: far(subwindow(4, 60, 3, True)), route("multi", block=256)),                 # trials in kb_solve_try<256>
    "multi_block256_wide": (lambda: far(subwindow(4, 150, 4, True)), route("multi", block=256, wt=1)),
    "multi_wide_trials": (lambda: far(subwindow(6, 100, 11, True), dp=0.03, dv=0.1), route("multi", wt=1)),
    "multi_wide_first": (lambda: far(subwindow(7, 240, 11, True), dp=0.03, dv=0.1), route("multi", wt=1, wf=1)),
    "multi_F33": (lambda: window(33, 40, 9, True, noise=30), route("multi", use_lds=0)),                  # trials in kb_solve_try<512>
}

# id: (problem, expected route, state rtol, what the oracle's trace of this problem must show)
CASES = {}


def _limited(make, m):
    return lambda: bh.with_max_iterations(make(), m)


def _add_series(name, make, expect):
    from oracle import ba_oracle as bo
    sm, tr = bo.solve_trace(bh.with_max_iterations(make(), 200), 512)
    p = bh.profile(tr, sm)
    # conditions of the route, on the oracle's side: a run of three or more rejections, which ends in convergence
    assert p["longest_run"] >= 3 and p["termination"] == CONVERGENCE and p["trailing_run"] >= 3, (name, p)
    m_rej, m_deep = bh.limit_values(tr)
    assert m_rej is not None and m_deep is not None and m_deep > m_rej, (name, m_rej, m_deep)
    CASES[name + "_m0"] = (_limited(make, 0), expect, 1e-7, dict(iterations=0, successes=0, termination=NO_CONVERGENCE))
    CASES[name + "_m1"] = (_limited(make, 1), expect, 1e-7, dict(iterations=1, termination=NO_CONVERGENCE))
    CASES[name + "_m2"] = (_limited(make, 2), expect, 1e-7, dict(iterations=2, termination=NO_CONVERGENCE))
    CASES[name + "_mrej"] = (_limited(make, m_rej), expect, 1e-7,
                             dict(iterations=m_rej, termination=NO_CONVERGENCE, limit_in_run=True, trailing=(1, 1)))
    CASES[name + "_mdeep"] = (_limited(make, m_deep), expect, 1e-7,
                              dict(iterations=m_deep, termination=NO_CONVERGENCE, limit_in_run=True, trailing=(2, 7)))
    CASES[name + "_m200"] = (_limited(make, 200), expect, 1e-7,
                             dict(termination=CONVERGENCE, longest_min=3, trailing=(3, 200), reason="parameter"))


for _name, (_make, _expect) in BASES.items():
    _add_series(_name, _make, _expect)
# the default limit on the single-launch routes: 30 iterations exhausted at the end of a rejection run
for _name in ("tiny", "chain_one_free", "chain_free3", "small_mid"):
    CASES[_name + "_m30"] = (BASES[_name][0], BASES[_name][1], 1e-7,
                             dict(iterations=30, termination=NO_CONVERGENCE, limit_in_run=True, longest_min=3))
# free landmarks (a Schur complement, depths that move with every candidate) on the wide routes: windows without the gauge prior, 30
# noise units out.  Only the limited solves: further on these windows grow the radius again, see the note on the choice of cases above
LANDMARKS = {
    "multi_wide_trials_landmarks": (lambda: window(6, 100, 5, False, fixed=1, noise=30), route("multi", wt=1)),
    "multi_wide_first_landmarks": (lambda: window(7, 200, 4, False, fixed=1, noise=30), route("multi", wt=1, wf=1)),
}


def _add_limited(name, make, expect):
    from oracle import ba_oracle as bo
    sm, tr = bo.solve_trace(bh.with_max_iterations(make(), 200), 512)
    m_rej, m_deep = bh.limit_values(tr)
    assert m_rej is not None and m_deep is not None and m_deep > m_rej, (name, m_rej, m_deep)
    CASES[name + "_mrej"] = (_limited(make, m_rej), expect, 1e-7,
                             dict(iterations=m_rej, termination=NO_CONVERGENCE, limit_in_run=True, trailing=(1, 1)))
    CASES[name + "_mdeep"] = (_limited(make, m_deep), expect, 1e-7,
                              dict(iterations=m_deep, termination=NO_CONVERGENCE, limit_in_run=True, trailing=(2, 7)))


for _name, (_make, _expect) in LANDMARKS.items():
    _add_limited(_name, _make, _expect)
# the gradient test before the first iteration (trial_begin's check_gradient, called from kb_tiny / kb_small_mid / kb_solve_try through
# try_block and from the wide-first kernels): cost and gradient zero at the start (prior only), and a stationary point with a cost
# above zero on every route that admits a prior (ba_hard.stationary).  kb_chain admits none: twelve oracle solves in a row, each from
# the last one's result, leave a gradient of 4 - 120 on both chain shapes, with and without their IMU factors (every solve stops by
# function tolerance, and moves the bias reference of the next) -- no stationary start was found for it.
_GRAD0 = dict(iterations=0, successes=0, termination=CONVERGENCE, reason="gradient")
CASES["tiny_grad0"] = (bh.prior_only, route("tiny"), 1e-7, _GRAD0)
CASES["multi_block256_prior_only_grad0"] = (lambda: bh.prior_only(3), route("multi", block=256), 1e-7, _GRAD0)
for _name, _make in (("tiny", lambda: one_free(4, 300, 3, True, j=2)), ("small_mid", lambda: one_free(4, 780, 3, True, j=2)),
                     ("multi_block256", lambda: subwindow(4, 60, 3, True)), ("multi_block256_wide", lambda: subwindow(4, 150, 4, True)),
                     ("multi_wide_trials", lambda: subwindow(6, 100, 11, True)), ("multi_wide_first", lambda: subwindow(7, 240, 11, True))):
    CASES[_name + "_stationary_grad0"] = ((lambda mk=_make: bh.stationary(mk())), BASES[_name][1], 1e-7, _GRAD0)

# every route has a case with three or more consecutive rejections, and one where the limit strikes inside such a run
for _name in BASES:
    assert CASES[_name + "_mdeep"][3]["trailing"][0] >= 2 and CASES[_name + "_m200"][3]["longest_min"] >= 3


@pytest.fixture(scope="module")
def ctx():
    from xrslam_amd import ba
    return ba.BaContext()


@pytest.fixture(scope="module")
def bo():
    from oracle import ba_oracle
    return ba_oracle


def _assert_route(ctx, pd, expect, case):
    d, got = dims(pd), ctx.debug_last_route()
    assert (got["na"], got["F"]) == (d["na"], d["F"]), (case, got, d)
    assert {k: got[k] for k in expect} == expect, (case, got)


@pytest.mark.parametrize("case", list(CASES))
def test_termination_parity(ctx, bo, case):
    make, expect, rtol, want = CASES[case]
    pd = make()
    sm, tr = bo.solve_trace(pd.copy(), 512)
    bh.check_profile(bh.profile(tr, sm), want, case)   # the case is what its name says, or it proves nothing
    sm_o, sm_h = solve_both(ctx, bo, pd, "term_" + case, rtol=rtol)
    _assert_route(ctx, pd, expect, case)
    assert sm_o.iterations == sm.iterations


# ---- saturated loss, landmarks behind the camera
SHAPES = {
    "na60": (lambda: window(5, 100, 7, False, fixed=1), route("multi", block=256, wt=1)),
    "na90_M600": (lambda: window(6, 200, 9, True), route("multi", wt=1, wf=1)),
    "na165": (lambda: window(11, 150, 2, True), route("multi", wt=1, wf=1)),
}
# (fraction of the observations moved, by how many pixels, every seventh depth negated)
OUTLIERS = [(0.1, 30, False), (0.1, 100, False), (0.3, 30, False), (0.3, 100, False), (0.3, 100, True)]


def _saturated(shape, frac, px, flip):
    return bh.saturated(SHAPES[shape][0](), frac, px, seed=int(100 * frac) + px, flip=flip)   # (asserts 20 observations at s > 100)


@pytest.mark.parametrize("frac,px,flip", OUTLIERS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_saturated_loss_solve_parity(ctx, bo, shape, frac, px, flip):
    pd = _saturated(shape, frac, px, flip)
    solve_both(ctx, bo, pd, "sat_%s_%d_%d_%d" % (shape, int(100 * frac), px, flip))
    _assert_route(ctx, pd, SHAPES[shape][1], shape)


@pytest.mark.parametrize("frac,px,flip", OUTLIERS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_saturated_loss_linearization_parity(ctx, bo, shape, frac, px, flip):
    pd = _saturated(shape, frac, px, flip)
    compare_linearization(ctx, bo, pd, "sat_%s_%d_%d_%d" % (shape, int(100 * frac), px, flip))


# ---- a cost that is not finite at the start: FAILURE, not usable, no iteration, the arrays bit for bit as passed; the context then solves
# an ordinary problem with full parity.  NaN / inf in the arrays are refused where xrhip_ba_solve stages them (nothing is launched);
# a finite 1e160 (the squared residuals overflow) and a zero inverse depth (0 / 0 in the reprojection) reach the device, where the first
# trial_begin of the solve stops on the non-finite cost.  Every device loop on the way there runs on an integer counter (for loops;
# the two `while (status == ST_RUNNING)` trial loops add 1 to `iteration` per pass; rounds and host guards count to
# 4 (max_iterations + 8)), and every kernel ends by publishing its sequence number.  One shape per route.
POISON = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "1e160": 1e160}
NF_SHAPES = dict(BASES, multi_wide_first_landmarks=LANDMARKS["multi_wide_first_landmarks"])


def _refused(pd, sms, solved):
    for sm in sms:
        assert (sm.termination, sm.usable, sm.iterations, sm.successful_steps) == (bh.FAILURE, 0, 0, 0)
        assert not np.isfinite(sm.initial_cost)
    for q in solved:
        assert q.frame_state.tobytes() == pd.frame_state.tobytes() and q.inv_depth.tobytes() == pd.inv_depth.tobytes()


@pytest.mark.parametrize("value", list(POISON))
@pytest.mark.parametrize("shape", ["tiny", "chain_free3", "small_mid", "multi_block256", "multi_wide_first", "multi_wide_first_landmarks"])
def test_nonfinite_start_is_refused(ctx, bo, shape, value):
    make, expect = NF_SHAPES[shape]
    pd = make()
    pd.frame_state[bh.free_frames(pd)[-1], 5] = POISON[value]
    a, b = pd.copy(), pd.copy()
    _refused(pd, (bo.solve(a), ctx.solve(b)), (a, b))
    if value == "1e160":
        _assert_route(ctx, pd, expect, shape)   # (it was the device that refused)
    good = bh.with_max_iterations(make(), 5)
    solve_both(ctx, bo, good, "after_nonfinite_" + shape)
    _assert_route(ctx, good, expect, shape)


@pytest.mark.parametrize("depth", [0.0, np.nan])
@pytest.mark.parametrize("shape", ["tiny", "chain_free3", "small_mid", "multi_block256", "multi_wide_first", "multi_wide_first_landmarks"])
def test_nonfinite_depth_of_an_observed_landmark_is_refused(ctx, bo, shape, depth):
    make, expect = NF_SHAPES[shape]
    pd = make()
    pd.inv_depth[pd.obs_lm[0]] = depth
    a, b = pd.copy(), pd.copy()
    _refused(pd, (bo.solve(a), ctx.solve(b)), (a, b))
    good = bh.with_max_iterations(make(), 5)
    solve_both(ctx, bo, good, "after_nonfinite_depth_" + shape)
    _assert_route(ctx, good, expect, shape)


def test_nonfinite_second_problem_of_a_linked_pair_is_refused(ctx, bo):
    """xrhip_ba_solve_chained (begin / linked / end, the pipeline's localize_newframe + refine_subwindow pair): a NaN in the second
    problem takes the pair off the one-submission path; the first solves as ever, the second is refused."""
    from xrslam_amd import ba
    second_ctx = ba.BaContext()
    first, second = one_free(4, 300, 3, False), subwindow(4, 60, 5, False)
    second.frame_state[2, 5] = np.nan
    want = first.copy()
    sm_o = bo.solve(want)
    a, b = first.copy(), second.copy()
    s1, s2 = ctx.solve_chained(a, 3, second_ctx, b, 3)
    assert (s1.iterations, s1.termination, s1.usable) == (sm_o.iterations, sm_o.termination, 1)
    np.testing.assert_allclose(a.frame_state, want.frame_state, rtol=1e-7, atol=1e-9)
    assert (s2.termination, s2.usable, s2.iterations, s2.successful_steps) == (bh.FAILURE, 0, 0, 0)
    assert b.frame_state[:3].tobytes() == second.frame_state[:3].tobytes()            # (frame 3 is the first solve's result)
    assert b.frame_state[3].tobytes() == a.frame_state[3].tobytes()
    second_ctx.close()
