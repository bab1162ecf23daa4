"""Scale-aware comparison of two marginalisation priors, shared by the CPU and the GPU tests.

A prior is (sqrt_info S, infovec iv); S and iv are defined up to an orthogonal transform, so two priors are compared on what the
solver consumes: Lambda = S^T S and eta = S^T iv.  Lambda spans many decades (rotation block ~1e8, accelerometer-bias diagonal ~1e4,
a kept gauge row 1e30), so a max-norm bound |dLambda| <= 1e-8 |Lambda|.max() says nothing about the small blocks.  Lambda is positive
semidefinite, |Lambda_ij| <= sqrt(Lambda_ii Lambda_jj), and eta_i = S[:, i] . iv is bounded by sqrt(Lambda_ii) |iv|; the deviations
are measured in those scalings, REF being the reference (the oracle):

    dLambda = max over the support of |Lambda_ij - REF_ij| / sqrt(REF_ii REF_jj)
    deta    = max over the support of |eta_i - REF_i| / (sqrt(REF_ii) |iv_REF|)

The support is where(diag(REF) > 0).  It must be the same set for both, and outside it the rows and columns of Lambda and the
entries of eta must be exactly zero (what km_support and the expansions of km_chol / km_jacobi promise, and what the oracle's Jacobi eigen-solver leaves).

Tolerances.  TOL[family] = 100 x the largest deviation of the ORACLE from an independent Schur complement carried out in np.longdouble
(tests/test_oracle_ba.py::_numpy_marginal) over the family's cases; measured on the CPU by
tests/test_oracle_ba.py::test_oracle_deviation_from_longdouble_is_what_the_tolerances_are_made_of, which also asserts that the
numbers below still hold.  Two decades: the device eliminates in another order (landmarks through the MFMA Schur product, then the
victim block) and factors differently (Cholesky where the oracle runs Jacobi).  Nothing here is derived from the device's output.

Oracle against longdouble, per case (dLambda, deta; R = unknowns of the new prior, `sup` = size of the support).  "K.. first" and
"K.. step n" are the windows of tests/test_ba_gpu.py::test_marginalization_parity (make_window(K, L, seed), victim 0, chained on the
oracle's own priors); the others are tests/marg_cases.py::CASES.

    family   case                      R  sup   dLambda    deta
    first    K6  L80  s22 first       75   39   4.2e-13   5.7e-15
    first    K11 L150 s21 first      150   69   3.6e-13   9.6e-15
    first    K16 L300 s23 first      225   99   3.3e-13   1.9e-14
    first    K21 L600 s24 first      300  129   2.7e-13   1.6e-14
    first    K35 L40  s25 first      510  213   3.9e-13   3.7e-14
    first    no_landmarks_first       75   15   4.1e-13   1.5e-15
    first    no_prior                 75   39   1.7e-12   6.9e-14
    chained  K6  step 1 / 2 / 3       60   33   2.4e-13   2.1e-14     (largest of the three steps)
    chained  K11 step 1 / 2 / 3      135   63   2.1e-13   1.2e-14
    chained  K16 step 1 / 2 / 3      210   93   1.5e-13   9.9e-15
    chained  K21 step 1 / 2 / 3      285  123   3.2e-13   1.3e-14
    chained  K35 step 1 / 2 / 3      495  207   4.9e-13   4.1e-14
    chained  chained_v2               60   51   3.8e-14   1.0e-14
    chained  chained_vlast            60   42   7.0e-12   1.3e-14
    chained  chained_k11_v2          135   81   5.1e-14   1.0e-14
    chained  chained_k11_vlast       135   72   3.5e-12   8.5e-15
    chained  chained3_k11_v2         105   69   3.9e-14   8.1e-15     (after three frame-0 marginalisations: the fast path)
    chained  subset_prior             90   45   2.2e-13   5.1e-15
    chained  no_landmarks_chained     60   33   2.2e-13   5.8e-15
    chained  unobserved_chained_v0    60   33   2.2e-13   5.8e-15
    gauge    first_v2                 75   48   1.0       2.9e-15
    gauge    first_vlast              75   39   1.0       1.8e-14
    gauge    unobserved_first_v2      75   36   1.0       1.1e-15

    family   tolerance dLambda   tolerance deta       (100 x the family's largest)
    first    1.7e-10             6.9e-12
    chained  7.0e-10             4.1e-12
    gauge    100 (asserts nothing)   1.8e-12

The "gauge" family (the victim is not frame 0 of a FIRST window, so make_window's 1e15 gauge rows on frame 0 stay in the result and
Lambda holds 1e30 beside 1e4) has no usable yardstick for Lambda: the oracle itself is a whole unit away from the Schur complement
there.  Its Jacobi eigen-solver (oracle/la.hpp sym_eigen) stops once the off-diagonal mass is below 1e-40 of the diagonal's, which
two 1e30 entries satisfy while the blocks below 1e10 are still undiagonalised; Lambda = V diag(w) V^T then lacks their off-diagonal
part.  (eta = V V^T b does not depend on how far the diagonalisation went, and is accurate.)  By the rule above the bound on dLambda
is 100, which no pair of positive semidefinite matrices can exceed: for this family the comparison holds the support, the exact
zeros outside it, eta and lin, and NOT Lambda.  That is a defect of the case's yardstick, recorded rather than papered over with a
bound picked by hand; the chained cases carry the victim != 0 shapes at a bound that bites.
"""
import numpy as np

# family -> cases -> (dLambda, deta) of the oracle against the longdouble Schur complement, as measured (rounded up to two digits)
MEASURED = {
    "first": {"K6_first": (4.2e-13, 5.7e-15), "K11_first": (3.6e-13, 9.6e-15), "K16_first": (3.3e-13, 1.9e-14),
              "K21_first": (2.7e-13, 1.6e-14), "K35_first": (3.9e-13, 3.7e-14), "no_landmarks_first": (4.1e-13, 1.5e-15),
              "no_prior": (1.7e-12, 6.9e-14)},
    "chained": {"K6_steps": (2.4e-13, 2.1e-14), "K11_steps": (2.1e-13, 1.2e-14), "K16_steps": (1.5e-13, 9.9e-15),
                "K21_steps": (3.2e-13, 1.3e-14), "K35_steps": (4.9e-13, 4.1e-14), "chained_v2": (3.8e-14, 1.0e-14),
                "chained_vlast": (7.0e-12, 1.3e-14), "chained_k11_v2": (5.1e-14, 1.0e-14), "chained_k11_vlast": (3.5e-12, 8.5e-15),
                "chained3_k11_v2": (3.9e-14, 8.1e-15),
                "subset_prior": (2.2e-13, 5.1e-15), "no_landmarks_chained": (2.2e-13, 5.8e-15),
                "unobserved_chained_v0": (2.2e-13, 5.8e-15)},
    "gauge": {"first_v2": (1.0, 2.9e-15), "first_vlast": (1.0, 1.8e-14), "unobserved_first_v2": (1.0, 1.1e-15)},
}

TOL = {fam: (100.0 * max(v[0] for v in cases.values()), 100.0 * max(v[1] for v in cases.values())) for fam, cases in MEASURED.items()}


def invariants(si, iv):
    return si.T @ si, si.T @ iv


def support(lam):
    return np.where(np.diag(lam) > 0)[0]


def old_maxnorm_accepts(lam, eta, lam_ref, eta_ref):
    """the comparison tests/test_ba_gpu.py::_marg_parity made before this metric (and still makes first)"""
    return bool(np.abs(lam - lam_ref).max() <= 1e-8 * np.abs(lam_ref).max() and
                np.abs(eta - eta_ref).max() <= 1e-7 * max(1.0, np.abs(eta_ref).max()))


def share_below_old_bound(lam):
    """the share of Lambda's non-zero entries that are smaller than the old max-norm bound itself"""
    nz = np.abs(lam[lam != 0])
    return float((nz < 1e-8 * nz.max()).mean())


def deviation(lam, eta, lam_ref, eta_ref, iv_norm):
    """-> dict(dlam, deta, sup, sup_ref, outside): the two scaled deviations over the reference's support, both supports, and the
    largest magnitude `lam` / `eta` hold outside the reference's support (0.0 when they are exactly zero there)"""
    lam, eta = np.asarray(lam, np.longdouble), np.asarray(eta, np.longdouble)
    ref, eref = np.asarray(lam_ref, np.longdouble), np.asarray(eta_ref, np.longdouble)
    sup_ref = support(ref)
    out = np.setdiff1d(np.arange(len(ref)), sup_ref)
    outside = 0.0
    if len(out):
        outside = float(max(np.abs(lam[out, :]).max(), np.abs(lam[:, out]).max(), np.abs(eta[out]).max()))
    s = np.sqrt(np.diag(ref)[sup_ref])
    dlam = np.abs(lam - ref)[np.ix_(sup_ref, sup_ref)] / np.outer(s, s) if len(sup_ref) else np.zeros((0, 0))
    if iv_norm > 0:
        deta = np.abs(eta - eref)[sup_ref] / (s * iv_norm)
    else:       # eta_ref is zero: nothing to scale by, only equality passes
        deta = np.where(eta[sup_ref] == eref[sup_ref], 0.0, np.inf)
    return dict(dlam=float(dlam.max()) if dlam.size else 0.0, deta=float(deta.max()) if deta.size else 0.0,
                sup=support(np.asarray(lam, np.float64)), sup_ref=sup_ref, outside=outside)


def check(lam, eta, lam_ref, eta_ref, iv_norm, tol, tag=""):
    """asserts the comparison of the module's docstring at tol = (tol_lambda, tol_eta); -> the deviation dict"""
    d = deviation(lam, eta, lam_ref, eta_ref, iv_norm)
    assert np.array_equal(d["sup"], d["sup_ref"]), "%s: support differs: %d rows against the reference's %d" % (
        tag, len(d["sup"]), len(d["sup_ref"]))
    assert d["outside"] == 0.0, "%s: %.3e outside the support" % (tag, d["outside"])
    assert d["dlam"] <= tol[0], "%s: dLambda %.3e > %.3e" % (tag, d["dlam"], tol[0])
    assert d["deta"] <= tol[1], "%s: deta %.3e > %.3e" % (tag, d["deta"], tol[1])
    return d


def accepts(lam, eta, lam_ref, eta_ref, iv_norm, tol):
    try:
        check(lam, eta, lam_ref, eta_ref, iv_norm, tol)
    except AssertionError:
        return False
    return True


def check_priors(si, iv, si_ref, iv_ref, family, tag=""):
    """two priors through the metric at the family's tolerance; -> the deviation dict"""
    lam, eta = invariants(si, iv)
    ref, eref = invariants(si_ref, iv_ref)
    return check(lam, eta, ref, eref, float(np.linalg.norm(iv_ref)), TOL[family], tag)


def predicted_path(lam):
    """What xrhip_ba_debug_marg_guard's status word [4] must be for a marginal matrix `lam`: 1 (the eigen path) when its support is
    rank deficient -- the smallest eigenvalue is a rounded zero, below 64 eps of the largest -- and 0 when the Cholesky fast path
    stands: km_chol's guard, 1 / trace(A^-1) on the support, is four decades above the 1e-8 eigenvalue floor.  None for a matrix in
    between: a case must not depend on which side of the gate rounding falls."""
    sup = support(lam)
    w = np.linalg.eigvalsh(lam[np.ix_(sup, sup)])
    if w[0] < 64 * np.finfo(np.float64).eps * w[-1]:
        return 1
    return 0 if 1.0 / np.sum(1.0 / w) > 1e-4 else None
