// ba_plan.hpp -- the code path of one bundle-adjustment solve, decided ONCE from the problem's sizes.
// plan_solve() is the only place that turns BaDims into a route, an LDS layout, a block size or a "wide" flag; every launch site
// of ba_api.hip reads the SolvePlan it returns, and xrhip_ba_debug_last_route reports that very plan (tests/test_ba_routes_gpu.py).
// Host only, no C ABI: tests/host_check/ba_plan_host.cpp pins the boundaries without a GPU (tests/test_ba_plan_host.py).
#pragma once
#include "../../include/xrslam_hip.h"
#include "ba_kernels.hip.h"
#include "ba_chain.hip.h"

#include <algorithm>
#include <cstdlib>

namespace xrhip {

// Development switches (A/B, parity) of the BA host side: each name is read here, once per process, and nowhere else.
struct BaSwitches {
    bool no_tiny = false;                 // XRHIP_NO_TINY: kb_tiny's problems take the multi-launch path
    bool no_chain = false;                // XRHIP_NO_CHAIN: the round-1 paths instead of kb_chain
    bool no_obs_cache = false;            // XRHIP_NO_OBS_CACHE: kb_chain without its table of per-solve constants
    bool no_tiled = false;                // XRHIP_NO_TILED: packed triangle instead of the tiled layouts
    bool no_spec = false;                 // XRHIP_NO_SPEC: no speculative linearisation of window solves
    bool group_spec = false;              // XRHIP_GROUP_SPEC: ... also for members of an instance group (instead of batched rounds)
    bool group_no_window_batch = false;   // XRHIP_GROUP_NO_WINDOW_BATCH: members launch their window rounds themselves
    bool no_chained_solves = false;       // XRHIP_NO_CHAINED_SOLVES: xrhip_ba_solve_begin queues nothing
    bool group_chained_solves = false;    // XRHIP_GROUP_CHAINED_SOLVES: ... does so for members of an instance group as well
};
inline const BaSwitches &ba_switches() {
    auto set = [](const char *name) { return std::getenv(name) != nullptr; };
    static const BaSwitches s = {set("XRHIP_NO_TINY"),   set("XRHIP_NO_CHAIN"),   set("XRHIP_NO_OBS_CACHE"),
                                 set("XRHIP_NO_TILED"),  set("XRHIP_NO_SPEC"),    set("XRHIP_GROUP_SPEC"),
                                 set("XRHIP_GROUP_NO_WINDOW_BATCH"), set("XRHIP_NO_CHAINED_SOLVES"), set("XRHIP_GROUP_CHAINED_SOLVES")};
    return s;
}

enum BaRoute { ROUTE_NONE = 0, ROUTE_TINY = 1, ROUTE_CHAIN = 2, ROUTE_SMALL_MID = 3, ROUTE_MULTI = 4 };   // (xrhip_ba_debug_last_route [0])

struct SolvePlan {
    int route = ROUTE_NONE;   // none: nothing free, nothing is launched
    int na = 0, F = 0;        // the sizes the plan was made for (free frame dofs, frames)
    // ROUTE_CHAIN: the whole solve in one LDS-resident launch (kb_chain)
    size_t chain_lds = 0;     // dynamic LDS: chain_layout() + the optional regions that fit
    int chain_opts = 0;       // CHAIN_OPT_*
    // the other routes: kb_tiny, or rounds of kb_solve_try (behind kb_small_mid: ROUTE_SMALL_MID, or behind the wide launches)
    int use_lds = -1;         // reduced system: 2 = tiled in LDS, 1 = packed triangle in LDS, 0 = factored in the global buffer
    int sred_tiled = 0;       // BaDims::sred_tiled: that global buffer is written and factored in the tiled layout, in place
    size_t try_lds = 0;       // dynamic LDS of kb_solve_try / kb_tiny (work region, at least the trials' TRY_B prior / IMU residuals)
    int block = 0;            // workgroup size of kb_solve_try, 256 or 512 (0: not launched)
    bool wide_trials = false; // a run of rejected trials goes to kb_trials_wide
    bool wide_first = false;  // ... and so does the first trial, queued right behind kb_solve_try
    size_t wide_lds = 0;      // dynamic LDS of kb_trials_wide
};

inline SolvePlan plan_solve(const BaDims &d, size_t lds_limit, const BaSwitches &sw) {
    SolvePlan pl;
    pl.na = d.na;
    pl.F = d.F;
    // ---- dynamic LDS of solve_block: work region = max(reduced system incl. the rhs row that rides along, gathered frame step of
    // the back-substitution); a system whose triangle does not fit is factored in the global buffer Sred instead
    const size_t tri = (size_t)(d.na + 1) * (d.na + 2) / 2;
    const size_t tiled = (size_t)tl_doubles(d.na + 1) + 16 * (size_t)tl_tile_rows(d.na + 1);   // tiles + L^-1 rhs
    const size_t aux = (size_t)d.PF;
    size_t lds = sizeof(double) * std::max(tiled, aux);
    int use_lds = 2;   // tiled layout (dense_lds.hip.h, round 3)
    if (sw.no_tiled || lds > lds_limit) {
        lds = sizeof(double) * std::max(tri, aux);
        use_lds = 1;   // packed triangle in LDS
    }
    if (lds > lds_limit) {
        use_lds = 0;   // in the global buffer, in the tiled layout (sred_tiled); L^-1 rhs / the solution in LDS
        lds = sizeof(double) * std::max(aux, (size_t)16 * tl_tile_rows(d.na + 1));
    }
    pl.sred_tiled = (use_lds == 0 && !sw.no_tiled) ? 1 : 0;

    // ---- no free landmark, no prior, a handful of free frames: the LDS-resident single-launch solve (ba_chain.hip.h)
    if (!sw.no_chain && d.nla == 0 && d.NP == 0 && d.nffp == 0 && d.na >= 1 && d.na <= CHAIN_MAX_NA && d.NI <= CHAIN_MAX_NI &&
        d.F <= CHAIN_MAX_F && d.M + d.MR <= CHAIN_MAX_OBS && d.nfree <= CHAIN_MAX_FREE) {
        size_t total = sizeof(double) * (size_t)chain_layout(d.F, d.na, d.NI, d.nfree, d.M + d.MR).total;
        if (total <= lds_limit) {
            // optional regions behind the layout, while they fit: the table of per-solve constants of the reprojection factors (the
            // bigger win: taken first when only one fits), then the reduction tile of the reprojection blocks
            const size_t tile = sizeof(double) * (size_t)CHAIN_VIS_TILE;
            const size_t cache = sizeof(double) * (size_t)CHAIN_OBS_CACHE * (size_t)chain_cache_stride(d.M);
            if (!sw.no_obs_cache && d.M > 0 && total + cache <= lds_limit) {
                pl.chain_opts |= CHAIN_OPT_CACHE;
                total += cache;
            }
            if (total + tile <= lds_limit) {
                pl.chain_opts |= CHAIN_OPT_TILE;
                total += tile;
            }
            pl.route = ROUTE_CHAIN;
            pl.chain_lds = total;
            return pl;
        }
    }
    pl.use_lds = use_lds;
    pl.try_lds = std::max(lds, sizeof(double) * (size_t)std::max(TRY_B * (d.np + 15 * d.NI), 1));
    // ---- small problems without a free landmark: assembly, preparation and the reduced system in one workgroup (kb_small_mid);
    // measured: beyond one free frame the wide launches win.  With few enough factors the whole trust-region loop runs inside one
    // launch (kb_tiny: localize_newframe and the initialiser's PnP WITH a prior).  Measured: with several free frames
    // (refine_subwindow, na = 30..60) the one-workgroup assembly of the active block (26 of its 41 us: ~60 dependent-latency loads
    // per entry, 8 entries per thread) costs more than the launches and round trips it saves (0.243 vs 0.215 ms per frame; index
    // tables in LDS did not change that).
    const bool small_mid = d.nla == 0 && d.na <= 16;
    if (small_mid && !sw.no_tiny && d.M + d.MR <= 640 && d.F <= 64) {   // kb_tiny lists the free frames in s_free[64]
        pl.route = ROUTE_TINY;
        return pl;
    }
    pl.route = small_mid ? ROUTE_SMALL_MID : ROUTE_MULTI;
    // Large problems hand a run of rejected trials to kb_trials_wide (the whole chip costs 8 candidates per launch); for small ones
    // the round trip would cost more than looping inside kb_solve_try ...
    pl.wide_trials = d.M >= 256 && d.F <= 32;
    // ... and window-sized problems (refine_window) cost even their first trial there
    pl.wide_first = pl.wide_trials && d.M >= 600 && d.na >= 90;
    // small problems (one observation per thread either way) run the 256-thread instance of kb_solve_try
    pl.block = (!pl.wide_first && d.M + d.MR <= 640 && d.na <= 64) ? 256 : 512;
    pl.wide_lds = sizeof(double) * ((size_t)WIDE_B * (16 * (size_t)d.F + (size_t)d.np) + (size_t)4 * WIDE_B * 257);
    return pl;
}

}   // namespace xrhip
