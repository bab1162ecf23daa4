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
