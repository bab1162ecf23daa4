"""Reference of the covariance tests (xrhip_ba_covariance): the cases, the reference inverse, a second CPU evaluation of it, and the
tolerance that follows from the two.

Reference: the oracle's dense H over all free dofs (orc_ba_linearize), Sigma_ref = np.linalg.inv(H), read through the returned
offsets.  Second evaluation: the Jacobi-scaled Schur complement of the same H in numpy, cholesky, triangular solves -- the route the
device takes, in LAPACK's summation order.  d_ref is the test's metric between the two; a case's tolerance is max(1e-9, 50 d_ref):
the error of either evaluation scales with the system's condition number, and the factor 50 covers the different summation order of
the matrix-core tiles.  Everything is computed once per case and cached; nobody modifies what is returned."""
import functools

import numpy as np

from xrslam_amd import abi

CASES = ("k2_fix0", "k3_prior", "k3_l1", "k3_l5", "k6", "k11", "k16", "k21", "k36_l40", "s1_window", "s2_window", "s3_window", "localize")
LANDMARK_CASES = ("k3_l1", "k3_l5", "k11", "s1_window")


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> abi.BaProblemData of the case (copy it before anything that writes)."""
    from tests import ba_snapshots, ba_synth as bs
    if name.endswith("_window"):
        return {n: pd for n, pd, _ in ba_snapshots.load_all()}[name]
    if name == "localize":
        return bs.make_localize()[0]
    if name == "k2_fix0":   # one free frame: na = 15, one tile, every padding path
        return bs.make_window(K=2, L=20, seed=3, with_prior=False, n_fixed_first=1)[0]
    # K = 3 with the prior and NOTHING fixed is rank deficient (two IMU intervals do not separate the accelerometer bias from gravity: the
    # smallest eigenvalue of the scaled H is -2e-16), so it cannot be a parity case; the K = 3 cases keep frame 0 constant (na = 30)
    spec = {"k3_prior": (3, 30, 1), "k3_l1": (3, 1, 1), "k3_l5": (3, 5, 1), "k6": (6, 40, 0), "k11": (11, 150, 0), "k16": (16, 60, 0),
            "k21": (21, 60, 0), "k36_l40": (36, 40, 0)}[name]
    return bs.make_window(K=spec[0], L=spec[1], seed=11 + spec[0], n_fixed_first=spec[2])[0]


def _maps(pd, po, mo):
    """frame-major index (15 f + k) -> local index of the oracle's H, -1 for a constant dof"""
    F = len(pd.frame_state)
    idx = -np.ones(15 * F, int)
    for f in range(F):
        if po[f] >= 0:
            idx[15 * f:15 * f + 6] = po[f] + np.arange(6)
        if mo[f] >= 0:
            idx[15 * f + 6:15 * f + 15] = mo[f] + np.arange(9)
    return idx


def _read(Sig, idx, lo, F):
    blocks = np.zeros((F, 15, 15))
    for f in range(F):
        ii = idx[15 * f:15 * f + 15]
        a = ii >= 0
        blocks[f][np.ix_(a, a)] = Sig[np.ix_(ii[a], ii[a])]
    var = np.array([Sig[l, l] if l >= 0 else 0.0 for l in lo])
    return blocks, var


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict(blocks [F][15][15], var [L], blocks2, var2 (the second evaluation), d_blocks [F], d_var [L], cond)"""
    from oracle import ba_oracle as bo
    pd = problem(name)
    F = len(pd.frame_state)
    _, H, _, po, mo, lo = bo.linearize(pd.copy())
    idx = _maps(pd, po, mo)
    blocks, var = _read(np.linalg.inv(H), idx, lo, F)
    # second evaluation: Schur complement over the frame dofs, Jacobi scaling, Cholesky, triangular solves
    fr = idx[idx >= 0]
    lm = np.array([l for l in lo if l >= 0], int)
    Hpp, hll = H[np.ix_(fr, fr)], np.diag(H)[lm] if len(lm) else np.zeros(0)
    W = H[np.ix_(lm, fr)] if len(lm) else np.zeros((0, len(fr)))
    S = Hpp - W.T @ (W / hll[:, None]) if len(lm) else Hpp
    d = 1.0 / np.sqrt(np.diag(S))
    Lc = np.linalg.cholesky(S * np.outer(d, d))
    Y = np.linalg.solve(Lc, np.eye(len(fr)))   # (no scipy here: a general solve on the triangular factor)
    Spp = (Y.T @ Y) * np.outer(d, d)
    Sig2 = np.zeros_like(H)
    Sig2[np.ix_(fr, fr)] = Spp
    for k, l in enumerate(lm):
        Sig2[l, l] = 1.0 / hll[k] + W[k] @ Spp @ W[k] / hll[k] ** 2
    blocks2, var2 = _read(Sig2, idx, lo, F)
    return dict(blocks=blocks, var=var, blocks2=blocks2, var2=var2, d_blocks=block_error(blocks2, blocks), d_var=var_error(var2, var),
                cond=float(np.linalg.cond(S * np.outer(d, d))), na=len(fr), nla=len(lm))


def block_error(got, ref):
    """relative Frobenius error per 15 x 15 block (0 where both are all zero)"""
    out = np.zeros(len(ref))
    for f in range(len(ref)):
        n = np.linalg.norm(ref[f])
        out[f] = np.linalg.norm(got[f] - ref[f]) / n if n > 0 else np.linalg.norm(got[f])
    return out


def var_error(got, ref):
    """relative error per variance (absolute where the reference is 0)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    return np.abs(got - ref) / np.where(ref != 0, np.abs(ref), 1.0)


def tolerance(name):
    """-> (tolerance of the blocks, tolerance of the variances) of the case: max(1e-9, 50 d_ref)"""
    r = reference(name)
    d_b = float(r["d_blocks"].max())
    d_v = float(r["d_var"].max()) if len(r["d_var"]) else 0.0
    return max(1e-9, 50 * d_b), max(1e-9, 50 * d_v)


def table():
    rows = ["| case | na | free landmarks | cond (scaled S) | d_ref blocks | d_ref variances | tol blocks | tol variances |", "|---|---|---|---|---|---|---|---|"]
    for name in CASES:
        r = reference(name)
        tb, tv = tolerance(name)
        rows.append("| %s | %d | %d | %.2e | %.2e | %.2e | %.2e | %.2e |" % (name, r["na"], r["nla"], r["cond"], r["d_blocks"].max(),
                                                                       r["d_var"].max() if len(r["d_var"]) else 0.0, tb, tv))
    return "\n".join(rows)
