// Host-side access to the solve plan of the bundle adjustment (xrslam_amd/csrc/ba_plan.hpp) for tests/test_ba_plan_host.py:
// the sizes go in field by field, the plan comes back as integers.  No development switch is set.
#include "../../xrslam_amd/csrc/ba_plan.hpp"

extern "C" void hc_ba_plan(int F, int M, int MR, int NI, int NP, int na, int nla, int nfree, int nffp, int lds_limit, long long *out10) {
    xrhip::BaDims d = {};
    d.F = F;
    d.n = 15 * F;
    d.PF = (6 * F + 15) / 16 * 16;
    d.M = M;
    d.MR = MR;
    d.NI = NI;
    d.NP = NP;
    d.np = 15 * NP;
    d.na = na;
    d.nla = nla;
    d.nfree = nfree;
    d.nffp = nffp;
    const xrhip::SolvePlan pl = xrhip::plan_solve(d, (size_t)lds_limit, xrhip::BaSwitches{});
    const long long v[10] = {pl.route,  pl.use_lds,     pl.sred_tiled, pl.block,         pl.wide_trials, pl.wide_first, (long long)pl.chain_lds,
                             pl.chain_opts, (long long)pl.try_lds, (long long)pl.wide_lds};
    for (int i = 0; i < 10; ++i) out10[i] = v[i];
}
