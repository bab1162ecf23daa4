"""The termination cases of tests/test_ba_termination_gpu.py replayed through the independent trust-region model (tests/tr_model.py):
the reference those GPU cases are held to is then two implementations that share no minimiser code, not the oracle alone.  Every
problem of that module's case table (same max_iterations) must give the oracle's record with the criteria tests/test_tr_model.py
applies to the frozen snapshots: iterations, accepted steps and termination; the accept / reject sequence, the radii and mu exactly;
costs to 1e-11, model terms to 1e-8, final states to atol 1e-11.  The model also names the test that ended the solve, which the
oracle's summary does not: the cases that claim the gradient test or the parameter tolerance are pinned to it here.  No GPU.

Where the two implementations stand on these cases (oracle against model, max_iterations = 200): costs 5e-14, model terms 5e-11,
final states 9e-16, radii and mu equal.  (How the cases were chosen so that radii CAN be equal: the GPU module's docstring.)"""
import numpy as np
import pytest

from oracle import ba_oracle as bo
from tests import ba_hard as bh
from tests import tr_model
from tests.test_ba_termination_gpu import CASES

# the 33-frame window: 535 dense unknowns and ~750 factors per evaluation in numpy, half a minute per solve -- the model's own
# test (tests/test_tr_model.py) and the six other routes cover the same decisions at K <= 8
SLOW = tuple(c for c in CASES if c.startswith("multi_F33"))


@pytest.mark.parametrize("case", [c for c in CASES if c not in SLOW])
def test_model_reproduces_the_oracle_record(case):
    make, _, _, want = CASES[case]
    pd = make()
    a, b = pd.copy(), pd.copy()
    sm, E = bo.solve_trace(a, 512)
    bh.check_profile(bh.profile(E, sm), want, case)
    trace = []
    out = tr_model.solve(b, trace=trace)
    assert out["iterations"] == sm.iterations
    assert out["successful_steps"] == sm.successful_steps
    assert out["termination"] == sm.termination and out["usable"] == sm.usable
    if "reason" in want:
        assert out["reason"] == want["reason"]
    if want.get("limit_in_run") or want.get("termination") == bh.NO_CONVERGENCE:
        assert out["reason"] == "limit"
    # (atol: the prior-only problem costs exactly 0 in the oracle and the square of a rounding error, 1e-30, in the model's quaternion
    # algebra; relative to the unit cost of a single one-sigma residual that is nothing)
    np.testing.assert_allclose(out["initial_cost"], sm.initial_cost, rtol=1e-12, atol=1e-24)
    np.testing.assert_allclose(out["final_cost"], sm.final_cost, rtol=1e-10, atol=1e-24)
    T = np.array(trace).reshape(-1, 9)
    assert T.shape == E.shape
    np.testing.assert_array_equal(T[:, 0], E[:, 0])                     # iteration numbers of the trials that reached a decision
    np.testing.assert_array_equal(T[:, 8], E[:, 8])                     # accepted / rejected
    np.testing.assert_array_equal(T[:, 5], E[:, 5])                     # trust-region radius at each trial (exact: halvings)
    np.testing.assert_array_equal(T[:, 7], E[:, 7])                     # mu
    np.testing.assert_allclose(T[:, 1], E[:, 1], rtol=1e-11)            # cost at x
    np.testing.assert_allclose(T[:, 2], E[:, 2], rtol=1e-11)            # cost at the candidate
    np.testing.assert_allclose(T[:, 3], E[:, 3], rtol=1e-8)             # model cost change (dense solve vs Schur elimination)
    np.testing.assert_allclose(T[:, 4], E[:, 4], rtol=1e-8)             # relative decrease
    np.testing.assert_allclose(T[:, 6], E[:, 6], rtol=1e-8)             # step norm (ambient coordinates)
    np.testing.assert_allclose(b.frame_state, a.frame_state, rtol=0, atol=1e-11)
    if len(pd.inv_depth):
        np.testing.assert_allclose(b.inv_depth, a.inv_depth, rtol=0, atol=1e-11)
