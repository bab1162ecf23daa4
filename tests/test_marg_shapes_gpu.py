"""GPU parity of the marginalisation (xrhip_ba_marginalize, the km_* kernels) against the CPU oracle on the shapes the frame-0 chain
of tests/test_ba_gpu.py does not reach (tests/marg_cases.py) and on the frozen problems the pipeline built
(tests/golden/marg_snapshots), in the scale-aware metric of tests/marg_metric.py.  The tolerances are that module's: 100 x what the
oracle itself differs by from a Schur complement in longdouble, measured on the CPU (tests/test_oracle_ba.py).

As measured on an MI355X when the tests were written (device against oracle; beside it the oracle against longdouble from
marg_metric's table; path = status word [4], 0 Cholesky fast path, 1 eigen path; no bound is derived from these):

    case                   path  support   dLambda  deta      oracle-vs-longdouble
    first_v2                1    48 of  75  1.0      3.9e-15   1.0      2.9e-15     (gauge family: Lambda is not held, see marg_metric)
    first_vlast             1    39 of  75  1.0      2.1e-14   1.0      1.8e-14
    unobserved_first_v2     1    36 of  75  1.0      3.1e-15   1.0      1.1e-15
    chained_v2              1    51 of  60  1.7e-14  3.4e-15   3.8e-14  1.0e-14
    chained_vlast           1    42 of  60  3.3e-13  1.4e-14   7.0e-12  1.3e-14
    chained_k11_v2          1    81 of 135  5.3e-14  4.0e-15   5.1e-14  1.0e-14
    chained_k11_vlast       1    72 of 135  1.1e-13  5.1e-15   3.5e-12  8.5e-15
    chained3_k11_v2         0    69 of 105  3.9e-14  5.9e-15   3.9e-14  8.1e-15
    subset_prior            0    45 of  90  2.4e-13  5.1e-15   2.2e-13  5.1e-15
    no_landmarks_chained    1    33 of  60  2.2e-13  3.4e-15   2.2e-13  5.8e-15
    unobserved_chained_v0   1    33 of  60  2.2e-13  3.4e-15   2.2e-13  5.8e-15
    snapshots s1/s2/s3 first   1   69 / 99 / 129   <= 4.5e-13  <= 3.6e-15
    snapshots steady, fewest   0   69 / 99 / 129   <= 1.6e-13  <= 1.3e-14
    no_landmarks_first      1    15 of  75  1.6e-13  2.2e-15   4.1e-13  1.5e-15
    no_prior                1    39 of  75  8.4e-13  5.4e-14   1.7e-12  6.9e-14     (both sides return a prior)"""
import numpy as np
import pytest

from tests import marg_cases as mc
from tests import marg_metric as mm
from tests.ba_parity import dump as _dump
from tests.ba_parity import solve_both as _solve_both

pytestmark = pytest.mark.gpu

PATHS = {}      # case -> status words of the device's marginalisation, for the test of the paths at the end of the module


@pytest.fixture(scope="module")
def ctx():
    from xrslam_amd import ba
    return ba.BaContext()


@pytest.fixture(scope="module")
def bo():
    from oracle import ba_oracle
    return ba_oracle


def _parity(ctx, bo, md, family, tag):
    """oracle against device on `md`: the metric at the family's tolerance, lin bit for bit; -> (status words, deviation, the
    device's prior)"""
    si_o, iv_o, lin_o = bo.marginalize(md)
    si_h, iv_h, lin_h = ctx.marginalize(md)
    st = ctx.marg_guard()[1]
    assert st[0] == 0, tag
    lam_o, eta_o = mm.invariants(si_o, iv_o)
    lam_h, eta_h = mm.invariants(si_h, iv_h)
    d = mm.deviation(lam_h, eta_h, lam_o, eta_o, float(np.linalg.norm(iv_o)))
    print("marg %-22s %-7s path %d  support %3d (oracle %3d) of %3d  dLambda %.2e  deta %.2e  outside %.1e  old-bound share %.2f" % (
        tag, family, st[4], len(d["sup"]), len(d["sup_ref"]), len(lam_o), d["dlam"], d["deta"], d["outside"],
        mm.share_below_old_bound(lam_o)))
    try:
        mm.check(lam_h, eta_h, lam_o, eta_o, float(np.linalg.norm(iv_o)), mm.TOL[family], tag)
    except AssertionError:
        _dump("marg_shape_mismatch_" + tag, Lo=lam_o, Lh=lam_h, eo=eta_o, eh=eta_h, ivo=iv_o, st=np.array(st))
        raise
    assert st[1] == len(d["sup"]), (tag, st)               # the support km_support counted is the one the result has
    np.testing.assert_array_equal(lin_h, lin_o, err_msg=tag)
    return st, d, (si_h, iv_h, lin_h)


def _device_chain(ctx, bo):
    """marg(md) for the builders of tests/marg_cases.py: every marginalisation a case is chained on runs on the device and is held to
    the oracle as well, and a solve of the window it leaves follows it, as in tests/test_ba_gpu.py's frame-0 chain"""
    def marg(md):
        family = "first" if np.abs(md.prior_sqrt_info).max() == 1e15 else "chained"
        return _parity(ctx, bo, md, family, "chain_step")[2]
    return marg


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_marginalization_shapes(ctx, bo, name):
    """Share of Lambda's non-zero entries below the OLD max-norm bound 1e-8 |Lambda|.max(), i.e. entries that bound could not see
    (oracle, CPU): victim 0 of the frame-0 chain 0.21 (K = 11, seed 21) and 0.29 (K = 6, seed 22), which is why the metric exists;
    first_v2 0.88, first_vlast 0.85 (the kept 1e30 gauge rows dwarf everything), chained_v2 0.28, chained_vlast 0.28,
    chained_k11_v2 0.20, chained_k11_vlast 0.20, chained3_k11_v2 0.05."""
    family, build = mc.CASES[name]
    md = build(_device_chain(ctx, bo))
    if name in ("first_v2", "first_vlast", "chained_v2", "chained_vlast", "chained_k11_v2", "chained_k11_vlast", "chained3_k11_v2"):
        assert md.victim != 0 and mc.has_foreign_reference(md)          # a landmark of the problem has ref != victim
        if name.endswith("vlast"):
            assert md.victim == len(md.frame_state) - 1 and len(md.imu_i) == 1
    if name.startswith("no_landmarks"):
        assert len(md.inv_depth) == 0 and len(md.obs_tgt) == 0
    if name.startswith("unobserved"):
        assert len(md.obs_tgt) == 0 and len(md.inv_depth) > 0
    if name == "no_prior":
        assert len(md.prior_frames) == 0
    st, d, _ = _parity(ctx, bo, md, family, name)
    assert 0 < len(d["sup"]) < 15 * (len(md.frame_state) - 1)
    if name == "subset_prior":
        assert len(md.prior_frames) == 5 and len(md.frame_state) == 7
        outside = np.concatenate([15 * f + np.arange(6, 15) for f in (4, 5)])      # window frames 5 and 6: velocity and biases
        assert not np.intersect1d(outside, d["sup"]).size
    # the path: what the marginal matrix itself demands (independent Schur complement, tests/test_oracle_ba.py::_numpy_marginal)
    from tests.test_oracle_ba import _numpy_marginal
    want = mm.predicted_path(_numpy_marginal(md)[0])
    assert want is not None, "the case sits on the gate between the two paths"
    assert st[4] == want, (name, st)
    PATHS[name] = st


def test_both_paths_are_reached_with_a_victim_that_is_not_frame_0(ctx, bo):
    """of the cases above with victim != 0, at least one stood on the Cholesky fast path ([4] == 0) and at least one took the eigen
    path ([4] == 1).  One frame-0 marginalisation does not yet give a victim in the middle a positive definite marginal (the first
    marginalisation's rank deficiency is still in the prior): chained_k11_v2 is the eigen path's; after three, chained3_k11_v2 is the
    fast path's."""
    for name in ("chained3_k11_v2", "chained_k11_v2", "chained_k11_vlast"):
        if name not in PATHS:               # (run on its own: the cases above have not been through this process)
            family, build = mc.CASES[name]
            PATHS[name] = _parity(ctx, bo, build(_device_chain(ctx, bo)), family, name)[0]
    assert PATHS["chained3_k11_v2"][4] == 0
    assert PATHS["chained_k11_v2"][4] == 1 and PATHS["chained_k11_vlast"][4] == 1


def test_workspace_that_moves_between_marginalisations(bo):
    """One context of its own: K = 2 (N = 30, R = 15: the scratch stays under the workspace's 1 MiB floor), K = 11 (N = 165, R = 150:
    about 1.3 MiB, so the workspace is reallocated and every buffer moves), K = 2 again in the larger block.  Each is a first window's
    frame-0 marginalisation (make_window(K, L, seed), moved off the prior's linearisation point), held to the oracle in the "first"
    family's tolerance like the cases above, and took the path its marginal matrix demands."""
    from tests.test_ba_stage_host import MARG_SCRATCH, scratch_expected
    from tests.test_oracle_ba import _numpy_marginal
    from xrslam_amd import ba
    assert scratch_expected(MARG_SCRATCH, 30, 15)[1] <= 1 << 20 < scratch_expected(MARG_SCRATCH, 165, 150)[1]
    small, large = mc.marg_problem(mc.first_window(2, 80, 22), 0), mc.marg_problem(mc.first_window(11, 150, 21), 0)
    c = ba.BaContext()
    try:
        for tag, md in (("k2", small), ("k11", large), ("k2_again", small)):
            assert 15 * (len(md.frame_state) - 1) == {"k2": 15, "k11": 150, "k2_again": 15}[tag]
            st, _, _ = _parity(c, bo, md, "first", "moving_" + tag)
            want = mm.predicted_path(_numpy_marginal(md)[0])
            assert want is not None and st[4] == want, (tag, st)
    finally:
        c.close()


@pytest.mark.parametrize("victim,n", [(2, 0), (5, 0), (2, 1), (4, 1)])
def test_window_left_by_a_marginalisation_off_frame_0_solves_as_the_oracles(ctx, bo, victim, n):
    """the generalised next window (tests/marg_cases.py::next_window: the victim gone with its observations and the IMU factors that
    touched it, the device's prior on the rest) through a solve on both sides, as the frame-0 chain does"""
    pd = mc.chained_window(ctx.marginalize, n=n) if n else mc.first_window()
    si, iv, lin = ctx.marginalize(mc.marg_problem(pd, victim))
    _solve_both(ctx, bo, mc.next_window(pd, victim, si, iv, lin), "after_marg_v%d_n%d" % (victim, n), rtol=1e-6)


def _expected_lambda(exp):
    sup, n = exp["support"], int(exp["size"])
    tri = np.zeros((len(sup), len(sup)))
    tri[np.triu_indices(len(sup))] = exp["lam_upper"]
    tri = tri + np.triu(tri, 1).T
    lam = np.zeros((n, n))
    lam[np.ix_(sup, sup)] = tri
    return lam


def test_pipeline_marginalisation_snapshots(ctx):
    """the frozen problems Pipeline's marginalize_frame built on the S1 / S2 / S3 streams (tests/golden/marg_snapshots: the first
    marginalisation, a steady-state one and the one with the fewest landmarks per stream) against the oracle's committed Lambda, eta
    and support.  Reads tests/golden only."""
    from tests import ba_snapshots
    snaps = ba_snapshots.load_all_marg()
    assert len(snaps) >= 3
    for name, md, exp in snaps:
        si, iv, lin = ctx.marginalize(md)
        st = ctx.marg_guard()[1]
        lam, eta = mm.invariants(si, iv)
        family = "first" if name.endswith("_first") else "chained"
        ref = _expected_lambda(exp)
        d = mm.deviation(lam, eta, ref, exp["eta"], float(exp["iv_norm"]))
        print("marg snapshot %-10s %-7s path %d  support %3d of %3d  dLambda %.2e  deta %.2e" % (
            name, family, st[4], len(d["sup"]), len(ref), d["dlam"], d["deta"]))
        try:
            mm.check(lam, eta, ref, exp["eta"], float(exp["iv_norm"]), mm.TOL[family], name)
        except AssertionError:
            _dump("marg_snapshot_mismatch_" + name, Lo=ref, Lh=lam, eo=exp["eta"], eh=eta, st=np.array(st))
            raise
        assert st[0] == 0 and st[1] == len(exp["support"]), (name, st)
        assert st[4] == mm.predicted_path(ref), (name, st)
        np.testing.assert_array_equal(lin, np.delete(md.frame_state, md.victim, axis=0), err_msg=name)
