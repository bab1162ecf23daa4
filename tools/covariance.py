"""Measures the covariance kernels (kc_factor, kc_selected_inverse, kc_landmark_var) with HIP events on the frozen window problems
s1_window, s2_window, s3_window and writes profiles/covariance.md: the case table of tests/cov_model.py (sizes, condition numbers,
tolerances, the 50-digit columns) with the errors and the rcond this GPU run gives beside it, and the times.

    python tools/covariance.py [--reps 20] [--out profiles/covariance.md]

Needs an MI355X.  The times are medians over the repetitions of one xrhip_ba_covariance call each (newest frame selected, with and
without landmark variances), taken with xrhip_ba_set_profiling on; nothing in the test suite depends on them."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance.md"))
    args = ap.parse_args()
    from tests import cov_model as cm
    from xrslam_amd import _lib, ba
    ctx = ba.BaContext()
    ctx._lib.xrhip_ba_set_profiling.argtypes = [C.c_void_p, C.c_int]
    ctx._lib.xrhip_ba_set_profiling(ctx._h, 1)
    # every case of the tests, all frames selected, with landmark variances: what the GPU gives against the reference the tests use
    measured = {}
    for name in cm.TABLE_CASES:
        pd = cm.problem(name).copy()
        F = len(pd.frame_state)
        out = ctx.covariance(pd, np.arange(F), landmarks=True)
        m = dict(status=out["status"], rcond=out["rcond"])
        if out["status"] == 0:
            hp = cm.reference_hp(name) if name in cm.HP_CASES else None
            ref = hp if hp is not None and hp["pd"] else cm.reference(name)
            m["err_blocks"] = float(cm.block_error(out["blocks"], ref["blocks"]).max())
            m["err_var"] = float(cm.var_error(out["var"], ref["var"]).max()) if len(ref["var"]) else 0.0
        measured[name] = m
    rows = []
    for name in ("s1_window", "s2_window", "s3_window"):
        pd = cm.problem(name).copy()
        F = len(pd.frame_state)
        for lm in (False, True):
            t = []
            for _ in range(args.reps + 2):
                out = ctx.covariance(pd, [F - 1], landmarks=lm)
                assert out["status"] == 0
                t.append(ctx.cov_times())
            ms = np.median(np.array(t[2:]), axis=0)
            r = cm.reference(name)
            rows.append("| %s | %d | %d | %s | %.4f | %.4f | %.4f | %.4f |" % (name, r["na"], r["nla"], "yes" if lm else "no", ms[0], ms[1],
                                                                          ms[2], ms[3]))
    # the cap: 64 free frames, na = 960 (timed on a window of its own with 60 landmarks; its parity cases are k64 and k64_fix0 above)
    from tests import ba_synth as bs
    big = bs.make_window(K=64, L=60, seed=75)[0]
    for lm in (False, True):
        t, status = [], None
        for _ in range(5):
            out = ctx.covariance(big, [63], landmarks=lm)
            status = out["status"]
            t.append(ctx.cov_times())
        ms = np.median(np.array(t[2:]), axis=0)
        rows.append("| synthetic K = 64 (status %d) | 960 | %d | %s | %.4f | %.4f | %.4f | %.4f |" % (
            status, int((big.landmark_fix == 0).sum()), "yes" if lm else "no", ms[0], ms[1], ms[2], ms[3]))
    text = ["# Covariance of window states and landmark depths (xrhip_ba_covariance)", "",
            "Written by tools/covariance.py on an MI355X, kernel revision %s." % _lib.kernel_revision(), "",
            "Every column headed \"GPU\" and every time below comes from that run; every other column is computed on the CPU",
            "(tests/cov_model.py) in the same run.", "",
            "## cases, tolerances and what the GPU gives", "",
            "Per case: d_ref is the test's metric between two CPU evaluations of the reference (np.linalg.inv of the oracle's H against the",
            "Jacobi-scaled Schur complement, cholesky and triangular solves in numpy); the GPU tests hold max(1e-9, 50 d_ref)",
            "(tests/cov_model.py; the d_ref of a run depends on the LAPACK build and its thread count in the last digits).  Where the",
            "order of H allows (<= about 130) the same quantities exist at 50 digits (mpmath): the error of either CPU evaluation against",
            "them, the pivot ratio of the Jacobi-scaled reduced system (what rcond estimates) and the relative error of numpy's own pivot",
            "ratio.  The ill_* rows are one window (K = 6, L = 12) behind a progressively weaker gauge prior; their tolerance is 50 times the",
            "Schur route's own error against the 50-digit reference plus 1e-12.",
            "",
            "GPU columns: all frames selected with landmark variances; the largest block and variance error against the 50-digit reference",
            "where the case has one, else against np.linalg.inv; rcond against the 50-digit pivot ratio (tolerance: 50 times numpy's own",
            "relative error plus 1e-12) or, for the large cases, against numpy's pivot ratio (tolerance 1e-6).", "",
            cm.table(measured=measured), "",
            "## kernel times", "",
            "HIP-event milliseconds, median of %d calls, newest frame selected.  \"whole call\" is the device work from the first launch of" % args.reps,
            "the linearisation to the last covariance kernel.  kc_selected_inverse includes the block gather of the landmark path.", "",
            "| problem | na | free landmarks | variances | kc_factor | kc_selected_inverse | kc_landmark_var | whole call |",
            "|---|---|---|---|---|---|---|---|"] + rows + [""]
    with open(args.out, "w") as fh:
        fh.write("\n".join(text))
    print("\n".join(text))


if __name__ == "__main__":
    main()
