"""Oracle parity of xrhip_ba_solve on every size route it can take, on both sides of every boundary between them.

xrhip_ba_solve picks its code path from the problem's size, once per solve (csrc/ba_plan.hpp: plan_solve).  Each case below builds a
problem just inside or just outside one of these decisions, asserts -- through xrhip_ba_debug_last_route, which reports the plan the
solve was launched from -- the route the solve actually took (a later change of a threshold or of the LDS limit must not quietly move
a case to the route next door), and holds the result to the oracle with the criteria of tests/ba_parity.py.  Where a route admits a
prior factor, it is run once with and once without one.  (tests/test_ba_plan_host.py pins the same boundaries on bare sizes, no GPU.)

  decision (SolvePlan)              source (csrc/)                         boundary
  route = chain, chain_lds          ba_plan.hpp plan_solve, ba_chain.hip.h no free landmark, no prior, nffp = 0, na <= 90,
                                                                           <= 6 free frames, NI <= 8, M + MR <= 1024, and
                                                                           chain_layout() within the 150 KiB of LDS
  route = tiny / small_mid          ba_plan.hpp plan_solve                 no free landmark, na <= 16; kb_tiny also M + MR <= 640
  block: kb_solve_try<256> / <512>  ba_plan.hpp plan_solve                 M + MR <= 640 and na <= 64 (and not wide_first)
  use_lds 2 / 1 / 0, try_lds        ba_plan.hpp plan_solve                 150 KiB of LDS: tiled up to na = 165, packed at 180,
                                                                           in the global buffer (tiled, in place) from 195
  tile grid of the tiled layout     dense_lds.hip.h tl_tile_rows(na + 1)   na = 255: the rhs row is the last row of the grid
  rhs gather of the in-place layout ba_kernels.hip.h factor_stage_tiled    na > 512: more unknowns than kb_solve_try's threads
  wide_trials                       ba_plan.hpp plan_solve                 M >= 256 and F <= 32
  wide_first                        ba_plan.hpp plan_solve                 wide_trials, M >= 600 and na >= 90
"""
import pytest

from tests.ba_hard import dims, one_free, route, subwindow, window
from tests.ba_parity import solve_both

pytestmark = pytest.mark.gpu

# id: (problem, expected route, state rtol).  M = reprojection factors, NI = IMU factors, na = free frame dofs, F = frames.
CASES = {
    # kb_tiny (M <= 640) vs kb_small_mid (M > 640): a prior, or NI = 9 > 8, keeps kb_chain out
    "tiny_prior_M639": (lambda: one_free(4, 750, 3, True), route("tiny"), 1e-7),
    "tiny_imu9_M618": (lambda: one_free(10, 700, 3, False, all_imu=True), route("tiny"), 1e-7),
    "small_mid_prior_M682": (lambda: one_free(4, 800, 3, True), route("small_mid", wt=1), 1e-7),
    "small_mid_imu9_M709": (lambda: one_free(10, 800, 3, False, all_imu=True), route("small_mid", wt=1), 1e-7),
    "chain_one_free_M682": (lambda: one_free(4, 800, 3, False), route("chain"), 1e-7),
    # kb_chain at 6 free frames and <= 1024 factors vs a prior, 7 free frames, > 1024 factors.  Its LDS layout (chain_layout) must
    # fit 150 KiB as well: at na = 90 that holds with five IMU factors (147 KiB at M = 977) but not with six (154 KiB)
    "chain_free6_NI5_M977": (lambda: subwindow(7, 240, 5, False, first_imu=False), route("chain"), 1e-7),
    "multi_free6_NI6_M977": (lambda: subwindow(7, 240, 5, False), route("multi", wt=1, wf=1), 1e-7),
    "multi_free6_prior_M977": (lambda: subwindow(7, 240, 5, True, first_imu=False), route("multi", wt=1, wf=1), 1e-7),
    "multi_free6_NI5_M1246": (lambda: subwindow(7, 300, 5, False, first_imu=False), route("multi", wt=1, wf=1), 1e-7),
    "multi_free7_M975": (lambda: subwindow(8, 200, 5, False), route("multi", wt=1, wf=1), 1e-7),
    "multi_free7_prior_M975": (lambda: subwindow(8, 200, 5, True), route("multi", wt=1, wf=1), 1e-7),
    # kb_solve_try<256> (na <= 64, M <= 640) vs <512>
    # (with the gauge prior and all four frames free the trust region stalls -- 30 iterations, 6 accepted -- and the final costs of
    # that walk part at 1.1e-8: frame 0 is held instead)
    "na60_prior": (lambda: window(5, 100, 7, True, fixed=1), route("multi", block=256, wt=1), 1e-7),
    "na60": (lambda: window(5, 100, 7, False, fixed=1), route("multi", block=256, wt=1), 1e-7),
    "na75_prior": (lambda: window(5, 100, 7, True), route("multi", wt=1), 1e-7),
    "na75": (lambda: window(6, 100, 7, False, fixed=1), route("multi", wt=1), 1e-7),
    # wide_first (M >= 600 and na >= 90) vs wide_trials only
    "na75_M600_prior": (lambda: window(5, 200, 9, True), route("multi", wt=1), 1e-7),
    "na90_prior": (lambda: window(6, 100, 9, True), route("multi", wt=1), 1e-7),
    "na90_M600_prior": (lambda: window(6, 200, 9, True), route("multi", wt=1, wf=1), 1e-7),
    "na90_M600": (lambda: window(7, 200, 9, False, fixed=1), route("multi", wt=1, wf=1), 1e-7),
    # use_lds: tiled in LDS up to 165 unknowns, packed triangle in LDS at 180, factored in place in the global buffer from 195;
    # at na = 255 the rhs row is the last row of the tile grid
    "na165_prior": (lambda: window(11, 150, 2, True), route("multi", wt=1, wf=1), 1e-7),
    "na165": (lambda: window(12, 150, 2, False, fixed=1), route("multi", wt=1, wf=1), 1e-7),
    "na180_prior": (lambda: window(12, 150, 4, True), route("multi", use_lds=1, wt=1, wf=1), 1e-7),
    "na180": (lambda: window(13, 150, 4, False, fixed=1), route("multi", use_lds=1, wt=1, wf=1), 1e-7),
    "na195_prior": (lambda: window(13, 150, 6, True), route("multi", use_lds=0, wt=1, wf=1), 1e-7),
    "na195": (lambda: window(14, 150, 6, False, fixed=1), route("multi", use_lds=0, wt=1, wf=1), 1e-7),
    "na240_prior": (lambda: window(16, 150, 8, True), route("multi", use_lds=0, wt=1, wf=1), 1e-7),
    "na240": (lambda: window(17, 150, 8, False, fixed=1), route("multi", use_lds=0, wt=1, wf=1), 1e-7),
    "na255_prior": (lambda: window(17, 150, 10, True), route("multi", use_lds=0, wt=1, wf=1), 1e-7),
    "na255": (lambda: window(18, 150, 10, False, fixed=1), route("multi", use_lds=0, wt=1, wf=1), 1e-7),
    # wide_trials needs F <= 32: a 33-frame window costs its trials inside kb_solve_try
    "F32_prior": (lambda: window(32, 40, 9, True), route("multi", use_lds=0, wt=1, wf=1), 1e-7),
    "F32": (lambda: window(32, 40, 9, False, fixed=1), route("multi", use_lds=0, wt=1, wf=1), 1e-7),
    "F32_M_below_600_prior": (lambda: window(32, 25, 9, True), route("multi", use_lds=0, wt=1), 1e-7),
    "F33_prior": (lambda: window(33, 40, 9, True), route("multi", use_lds=0), 1e-7),
    "F33": (lambda: window(33, 40, 9, False, fixed=1), route("multi", use_lds=0), 1e-7),
    # past one kb_solve_try thread per unknown (512)
    "na510_prior": (lambda: window(34, 40, 11, True), route("multi", use_lds=0), 1e-7),
    "na510": (lambda: window(35, 40, 11, False, fixed=1), route("multi", use_lds=0), 1e-7),
    "na525_prior": (lambda: window(35, 40, 12, True), route("multi", use_lds=0), 1e-7),
    "na525": (lambda: window(36, 40, 12, False, fixed=1), route("multi", use_lds=0), 1e-7),
    "na600_prior": (lambda: window(40, 40, 13, True), route("multi", use_lds=0), 1e-7),
    "na600": (lambda: window(41, 40, 13, False, fixed=1), route("multi", use_lds=0), 1e-7),
}


@pytest.fixture(scope="module")
def ctx():
    from xrslam_amd import ba
    return ba.BaContext()


@pytest.fixture(scope="module")
def bo():
    from oracle import ba_oracle
    return ba_oracle


@pytest.mark.parametrize("case", list(CASES))
def test_solve_route_parity(ctx, bo, case):
    make, expect, rtol = CASES[case]
    pd = make()
    d = dims(pd)
    solve_both(ctx, bo, pd, "route_" + case, rtol=rtol)
    got = ctx.debug_last_route()
    assert (got["na"], got["F"]) == (d["na"], d["F"]), (case, got, d)
    assert {k: got[k] for k in expect} == expect, (case, got)
