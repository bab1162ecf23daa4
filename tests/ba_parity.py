"""Oracle parity of a bundle-adjustment solve, shared by the GPU test modules: the HIP solve (C ABI) against the CPU oracle on the
same problem."""
import os

import numpy as np

DUMP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")


def dump(name, **arrs):
    try:
        os.makedirs(DUMP, exist_ok=True)
        np.savez_compressed(os.path.join(DUMP, name + ".npz"), **arrs)
    except Exception:
        pass


def compare_linearization(ctx, bo, pd, tag):
    """xrhip_ba_debug_linearize against the oracle's normal equations at pd's state: cost to 1e-10, H per element to 1e-6 of
    max(|H_ij|, 1e-6 sqrt(H_ii H_jj)), gradient to 1e-8 of its largest entry."""
    cost_o, H_o, g_o, po, mo, lo = bo.linearize(pd)
    dev = ctx.debug_linearize(pd)
    F, Ln = len(pd.frame_state), len(pd.inv_depth)
    n_local = H_o.shape[0]
    # map the oracle's compact local layout to frame-major + landmarks
    idx = -np.ones(15 * F + Ln, int)
    for f in range(F):
        if po[f] >= 0:
            idx[15 * f:15 * f + 6] = po[f] + np.arange(6)
        if mo[f] >= 0:
            idx[15 * f + 6:15 * f + 15] = mo[f] + np.arange(9)
    for l in range(Ln):
        if lo[l] >= 0:
            idx[15 * F + l] = lo[l]
    full = np.zeros((15 * F + Ln, 15 * F + Ln))
    gfull = np.zeros(15 * F + Ln)
    act = idx >= 0
    full[np.ix_(act, act)] = H_o[np.ix_(idx[act], idx[act])]
    gfull[act] = g_o[idx[act]]
    n = 15 * F
    Hd = np.zeros_like(full)
    Hd[:n, :n] = dev["H"]
    pose_cols = np.concatenate([15 * f + np.arange(6) for f in range(F)])
    for l in range(Ln):
        Hd[n + l, n + l] = dev["hll"][l] if act[n + l] else 0.0
        Hd[pose_cols, n + l] = dev["W"][l]
        Hd[n + l, pose_cols] = dev["W"][l]
    gd = np.concatenate([dev["g"], np.where(act[n:], dev["gl"], 0.0)])
    scale = np.abs(full).max()
    ok = (abs(dev["cost"] - cost_o) <= 1e-10 * max(1.0, abs(cost_o)) and np.abs(Hd - full).max() <= 1e-9 * scale and
          np.abs(gd - gfull).max() <= 1e-9 * max(1.0, np.abs(gfull).max()))
    if not ok:
        dump("ba_lin_mismatch_" + tag, Hd=Hd, Ho=full, gd=gd, go=gfull, cost=np.array([dev["cost"], cost_o]))
    assert abs(dev["cost"] - cost_o) <= 1e-10 * max(1.0, abs(cost_o))
    # 1e15 gauge prior entries (1e30 in H) need a relative comparison per element
    denom = np.maximum(np.abs(full), 1e-6 * np.sqrt(np.outer(np.abs(np.diag(full)) + 1e-300, np.abs(np.diag(full)) + 1e-300)))
    assert (np.abs(Hd - full) / np.maximum(denom, 1e-300)).max() < 1e-6
    assert np.abs(gd - gfull).max() <= 1e-8 * max(1.0, np.abs(gfull).max())


def solve_both(ctx, bo, pd, tag, rtol=1e-7):
    a, b = pd.copy(), pd.copy()
    sm_o = bo.solve(a)
    sm_h = ctx.solve(b)
    good = (sm_o.iterations == sm_h.iterations and sm_o.termination == sm_h.termination and
            np.allclose(a.frame_state, b.frame_state, rtol=rtol, atol=1e-9) and
            np.allclose(a.inv_depth, b.inv_depth, rtol=rtol, atol=1e-9))
    if not good:
        dump("ba_solve_mismatch_" + tag, so=a.frame_state, sh=b.frame_state, do=a.inv_depth, dh=b.inv_depth,
             meta=np.array([sm_o.iterations, sm_h.iterations, sm_o.termination, sm_h.termination,
                            sm_o.successful_steps, sm_h.successful_steps, sm_o.final_cost, sm_h.final_cost,
                            sm_o.initial_cost, sm_h.initial_cost]))
    assert abs(sm_h.initial_cost - sm_o.initial_cost) <= 1e-9 * sm_o.initial_cost
    assert sm_h.iterations == sm_o.iterations and sm_h.successful_steps == sm_o.successful_steps
    assert sm_h.termination == sm_o.termination and sm_h.usable == sm_o.usable
    # north_star tolerance: 1e-4 relative on pose/velocity/bias states; assert much tighter
    np.testing.assert_allclose(b.frame_state, a.frame_state, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(b.inv_depth, a.inv_depth, rtol=rtol, atol=1e-9)
    assert abs(sm_h.final_cost - sm_o.final_cost) <= 1e-8 * sm_o.final_cost
    return sm_o, sm_h
