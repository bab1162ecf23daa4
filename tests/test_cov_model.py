"""CPU: the two evaluations of the covariance reference (tests/cov_model.py) agree to 1e-6 on every case the GPU tests use, so each
case's tolerance max(1e-9, 50 d_ref) tests something; a case too ill-conditioned for that is replaced, not loosened.  The cases added
for the cap, the partly constant frames, the landmark edges and the ill-conditioned family hold the conditions they were chosen for:
definiteness, sizes, the band of the condition number, and -- where there is one -- the 50-digit reference."""
import numpy as np
import pytest

from tests import cov_model as cm


@pytest.mark.parametrize("name", cm.CASES + cm.PARTIAL_CASES + cm.EDGE_CASES)
def test_reference_evaluations_agree(name):
    r = cm.reference(name)
    print("%s: na %d, free landmarks %d, cond %.3e, d_ref blocks %.3e, variances %.3e" % (
        name, r["na"], r["nla"], r["cond"], r["d_blocks"].max(), r["d_var"].max() if len(r["d_var"]) else 0.0))
    assert r["d_blocks"].max() < 1e-6
    if len(r["d_var"]):
        assert r["d_var"].max() < 1e-6
    for f in range(len(r["blocks"])):
        assert np.all(np.diag(r["blocks"][f]) >= 0)


@pytest.mark.parametrize("name", sorted(cm.EXPECTED, key=list(cm.TABLE_CASES).index))
def test_new_case_is_what_was_tabulated(name):
    """H positive definite (Cholesky of the Jacobi-scaled H, and its smallest eigenvalue), na, n16 and the free landmarks as tabulated,
    cond(scaled S) within a factor of 3 of the value the case was chosen at."""
    na, n16, nla, cond = cm.EXPECTED[name]
    H = cm.linearized(name)[0]
    r = cm.reference(name)
    d = 1.0 / np.sqrt(np.diag(H))
    assert np.all(np.diag(H) > 0)
    if name in cm.ILL_CASES:   # (doubles cannot tell below cond ~ 1e14: the 50-digit factorisation decides)
        assert cm.reference_hp(name)["pd"]
    else:
        np.linalg.cholesky(H * np.outer(d, d))
        assert np.linalg.eigvalsh(H * np.outer(d, d))[0] > 0
    print("%s: na %d, free landmarks %d, cond %.3e" % (name, r["na"], r["nla"], r["cond"]))
    assert (r["na"], 16 * ((r["na"] + 15) // 16), r["nla"]) == (na, n16, nla)
    assert cond / 3 <= r["cond"] <= 3 * cond


@pytest.mark.parametrize("name", cm.LARGE_CASES)
def test_large_case_tolerance_is_the_floor(name):
    """d_ref <= 2e-11: the tolerance of a case at the cap is the 1e-9 floor, nothing a wrong kernel could hide in."""
    r = cm.reference(name)
    assert r["d_blocks"].max() <= 2e-11 and r["d_var"].max() <= 2e-11
    assert cm.tolerance(name) == (1e-9, 1e-9)
    assert r["cond"] <= 4e5 and cm.factorable(name)   # (what rcond_tolerance's 1e-6 rests on)


def test_partial_cases_put_constant_slots_where_they_were_meant():
    """k5_straddle: a FIX_MOTION frame and a FIX_POSE frame whose free dofs lie across a multiple of 16 in the reduced order (frame-major,
    pose before motion); k6_fixpose0 and k5_straddle: na is no multiple of 15; every partial case has a one-bit frame before its last."""
    from xrslam_amd import abi
    fix = cm.problem("k5_straddle").frame_fix
    r, across = 0, {}
    for f, b in enumerate(fix):
        n = 15 - (6 if b & abi.FIX_POSE else 0) - (9 if b & abi.FIX_MOTION else 0)
        if b and n and r // 16 != (r + n - 1) // 16:
            across[int(b)] = (f, r, r + n - 1)
        r += n
    assert set(across) == {abi.FIX_POSE, abi.FIX_MOTION}, across
    assert cm.reference("k6_fixpose0")["na"] % 15 != 0 and cm.reference("k5_straddle")["na"] % 15 != 0
    for name in cm.PARTIAL_CASES:   # a frame with one bit alone, and frames after it (their columns shift by 6 or 9, not 15)
        fix = cm.problem(name).frame_fix
        assert any(b in (abi.FIX_POSE, abi.FIX_MOTION) for b in fix[:-1])


@pytest.mark.parametrize("name", cm.HP_CASES)
def test_hp_reference(name):
    """The 50-digit reference exists, both double evaluations lie within 1e-6 of it where cond <= 1e9 (so it is the same quantity, read
    through the same maps), and its pivot ratio is numpy's to the accuracy cond allows."""
    h, r = cm.reference_hp(name), cm.reference(name)
    assert h["pd"]
    print("%s: cond %.3e, inv vs 50 digits %.3e / %.3e, Schur route %.3e / %.3e, rcond %.6e (numpy off by %.3e)" % (
        name, r["cond"], h["err_blocks"], h["err_var"], h["err2_blocks"], h["err2_var"], h["rcond"], h["rcond_np_err"]))
    assert 0 < h["piv_min"] <= h["piv_max"] <= 1 + 1e-12
    assert np.array_equal(h["var"] == 0, r["var"] == 0) and np.array_equal(h["blocks"] == 0, r["blocks"] == 0)
    if r["cond"] <= 1e9:
        assert max(h["err_blocks"], h["err_var"], h["err2_blocks"], h["err2_var"]) < 1e-6
        assert h["rcond_np_err"] < 1e-6


def test_ill_family():
    """cond(scaled S) rises through the family; at least three members are positive definite at 50 digits with cond between 1e9 and
    1e13; at most one member is not positive definite at 50 digits (the only ground on which the GPU test may leave one unmeasured); the
    numpy route's own error against the 50-digit reference is finite wherever numpy's Cholesky succeeds, and it is recorded (-s)."""
    conds = [cm.reference(n)["cond"] for n in cm.ILL_CASES]
    hp = [cm.reference_hp(n) for n in cm.ILL_CASES]
    assert all(b > a for a, b in zip(conds, conds[1:]))
    assert sum(1 for c, h in zip(conds, hp) if h["pd"] and 1e9 <= c <= 1e13) >= 3
    assert sum(1 for h in hp if not h["pd"]) <= 1
    for n, c, h in zip(cm.ILL_CASES, conds, hp):
        if not h["pd"]:
            continue
        tb, tv = cm.tolerance_hp(n)
        print("%s: cond %.3e, Schur route vs 50 digits %.3e / %.3e, inv %.3e / %.3e, tolerance %.3e / %.3e, factorable %s" % (
            n, c, h["err2_blocks"], h["err2_var"], h["err_blocks"], h["err_var"], tb, tv, cm.factorable(n)))
        if cm.reference(n)["blocks2"] is not None:
            assert np.isfinite(h["err2_blocks"]) and np.isfinite(h["err2_var"]) and tb < 1 and tv < 1
    assert sum(1 for n in cm.ILL_CASES if cm.factorable(n)) >= 4


def test_edge_cases_are_the_edges():
    """The lonely landmark's row of W has no free entry, so its variance is 1 / hll; L % 4 is 1, 2, 3; the last landmark is free; the
    last group of four holds a constant landmark next to a free one where it has two or more."""
    for name in cm.EDGE_CASES:
        pd, r = cm.problem(name), cm.reference(name)
        H, idx, lo, fr, lm = cm.linearized(name)
        L = len(pd.inv_depth)
        assert L % 4 == {"edge_l9": 1, "edge_l10": 2, "edge_l11": 3}[name]
        assert lo[cm.EDGE_LONELY] >= 0 and not np.any(H[lo[cm.EDGE_LONELY], fr])
        assert abs(r["var"][cm.EDGE_LONELY] * r["hll"][cm.EDGE_LONELY] - 1.0) <= 1e-13
        assert abs(cm.reference_hp(name)["var"][cm.EDGE_LONELY] * r["hll"][cm.EDGE_LONELY] - 1.0) <= 1e-15
        assert r["var"][L - 1] > 1.0 / r["hll"][L - 1] > 0
        last = np.arange(4 * ((L - 1) // 4), L)
        if len(last) >= 2:
            assert np.any(r["var"][last] == 0) and np.count_nonzero(r["var"][last]) >= 1


def test_unanchored_last_frame_has_a_zero_diagonal():
    """cm.unanchored_last_frame: the oracle's H is exactly 0 on the last frame's 15 dofs and positive on every other frame dof."""
    from oracle import ba_oracle as bo
    pd = cm.unanchored_last_frame()
    _, H, _, po, mo, lo = bo.linearize(pd.copy())
    assert po[5] >= 0 and mo[5] >= 0
    dg = np.diag(H)
    assert np.all(dg[po[5]:po[5] + 6] == 0) and np.all(dg[mo[5]:mo[5] + 9] == 0)
    for f in range(5):
        assert np.all(dg[po[f]:po[f] + 6] > 0) and np.all(dg[mo[f]:mo[f] + 9] > 0)


def test_table_prints():
    t = cm.table()
    print(t)
    assert t.count("\n") == len(cm.TABLE_CASES) + 1
