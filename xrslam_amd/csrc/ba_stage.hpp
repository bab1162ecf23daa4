// ba_stage.hpp -- the device layout of one staged bundle-adjustment problem, written down ONCE.
// stage_index() builds the gather tables on the host; XRHIP_BA_LAYOUT lists every buffer of the input arena and of the device workspace
// with its size; offsets and totals, the BaPtrs of a solve, the copies into the pinned arena, the second pointer set of a speculative
// linearisation and the exchange of the two sets are all expansions of that one list.  Behind it the three scratch layouts that are
// not a staged problem's -- marg_scratch (marginalisation, work2), cov_scratch (xrhip_ba_covariance) and preint_scratch (the pinned
// block of a pre-integration batch) -- and marg_problem_view, the marginalisation's factors as a BA problem.  ba_api.hip keeps what
// needs the HIP runtime.
// Host only, no C ABI: tests/host_check/ba_stage_host.cpp pins offsets, sets and tables without a GPU (tests/test_ba_stage_host.py).
#pragma once
#include "../../include/xrslam_hip.h"
#include "ba_kernels.hip.h"
#include "ba_plan.hpp"
#include "marg_kernels.hip.h"   // PreintJob
#include "cov_kernels.hip.h"    // CovStatus (after marg_kernels.hip.h, as ba_api.hip includes them: the order is part of the build)

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace xrhip {

// One staged solve as its launches see it: the argument block that travels with the problem (d, p, cam, imu, sx, sy) and the plan
// made from its sizes.  A linearisation at another buffer set is the same value with `p` replaced.
struct Staged : TinyArgs {
    SolvePlan pl;
};

// The bump every arena here uses: the next 256-byte boundary, at least 8 bytes taken.  Returns the offset, advances `used`.
inline size_t bump256(size_t &used, size_t bytes) {
    const size_t off = (used + 255) & ~size_t(255);
    used = off + std::max(bytes, size_t(8));
    return off;
}

// ---------------------------------------------------------------------------------------------- gather tables
struct StageIndex {
    std::vector<uint8_t> lact;                 // [L] landmark is a free parameter
    std::vector<int> lm_start, lm_obs;         // CSR landmark -> observations
    std::vector<int> pair_start, pair_items;   // CSR (row frame, col frame) -> (obs << 1 | role)
    std::vector<int> rotf_start, rotf_items;   // CSR frame -> rotation factors
    std::vector<int> act_idx, act_inv;         // free frame dofs, and their inverse
    std::vector<int> imuf, priorf;             // [F][2] IMU factor that ends / starts at the frame, [F] index in prior_frames
    std::vector<double> bias_ref;              // [NI][6] the biases the IMU factors were integrated at
};

// Counts the problem into `d` (every field but sred_tiled, which the plan decides) and builds the tables.  Returns the reason of a
// refusal, or null.  The problem's indices are in range (validate() in ba_api.hip).
inline const char *stage_index(const xrhip_ba_problem *P, int schur_mode, BaDims &d, StageIndex &ix) {
    d = BaDims{};
    d.F = P->n_frames;
    d.n = 15 * d.F;
    d.PF = (6 * d.F + 15) / 16 * 16;
    d.L = P->n_landmarks;
    d.Lp = std::max(16, (d.L + 15) / 16 * 16);
    d.M = P->n_obs;
    d.MR = P->n_rot;
    d.NI = P->n_imu;
    d.NP = P->prior_n;
    d.np = 15 * d.NP;
    d.NV = d.n + d.L;
    d.robust = 1;
    d.schur_mode = schur_mode;
    const int F = d.F, L = d.L, M = d.M, MR = d.MR, NI = d.NI, NP = d.NP;

    ix.lact.assign(std::max(L, 1), 0);
    for (int o = 0; o < M; ++o) ix.lact[P->obs_lm[o]] = 1;
    for (int l = 0; l < L; ++l)
        if (P->landmark_fix && P->landmark_fix[l]) ix.lact[l] = 0;
    ix.lm_start.assign(L + 1, 0);
    ix.lm_obs.assign(std::max(M, 1), 0);
    for (int o = 0; o < M; ++o) ix.lm_start[P->obs_lm[o] + 1]++;
    for (int l = 0; l < L; ++l) ix.lm_start[l + 1] += ix.lm_start[l];
    {
        std::vector<int> fill(ix.lm_start.begin(), ix.lm_start.end() - 1);
        for (int o = 0; o < M; ++o) ix.lm_obs[fill[P->obs_lm[o]]++] = o;
    }
    ix.pair_start.assign((size_t)F * F + 1, 0);
    ix.pair_items.assign(std::max(4 * M, 1), 0);
    auto pair_count = [&](int a, int b) { ix.pair_start[(size_t)a * F + b + 1]++; };
    for (int o = 0; o < M; ++o) {
        const int t = P->obs_tgt[o], r = P->obs_ref[o];
        pair_count(t, t);
        pair_count(r, r);
        pair_count(t, r);
        pair_count(r, t);
    }
    for (size_t i = 0; i < (size_t)F * F; ++i) ix.pair_start[i + 1] += ix.pair_start[i];
    {
        std::vector<int> fill(ix.pair_start.begin(), ix.pair_start.end() - 1);
        for (int o = 0; o < M; ++o) {
            const int t = P->obs_tgt[o], r = P->obs_ref[o];
            ix.pair_items[fill[(size_t)t * F + t]++] = (o << 1) | 0;
            ix.pair_items[fill[(size_t)r * F + r]++] = (o << 1) | 1;
            ix.pair_items[fill[(size_t)t * F + r]++] = (o << 1) | 0;
            ix.pair_items[fill[(size_t)r * F + t]++] = (o << 1) | 1;
        }
    }
    ix.rotf_start.assign(F + 1, 0);
    ix.rotf_items.assign(std::max(MR, 1), 0);
    for (int o = 0; o < MR; ++o) ix.rotf_start[P->rot_tgt[o] + 1]++;
    for (int f = 0; f < F; ++f) ix.rotf_start[f + 1] += ix.rotf_start[f];
    {
        std::vector<int> fill(ix.rotf_start.begin(), ix.rotf_start.end() - 1);
        for (int o = 0; o < MR; ++o) ix.rotf_items[fill[P->rot_tgt[o]]++] = o;
    }
    ix.act_idx.clear();
    for (int a = 0; a < 15 * F; ++a) {
        const int f = a / 15, k = a % 15;
        if (k < 6 ? !(P->frame_fix[f] & XRHIP_FIX_POSE) : !(P->frame_fix[f] & XRHIP_FIX_MOTION)) ix.act_idx.push_back(a);
    }
    d.na = (int)ix.act_idx.size();
    ix.act_inv.assign((size_t)15 * F, -1);
    for (size_t i = 0; i < ix.act_idx.size(); ++i) ix.act_inv[ix.act_idx[i]] = (int)i;
    d.nla = 0;
    for (int l = 0; l < L; ++l) d.nla += ix.lact[l] ? 1 : 0;
    d.lm_rows = d.Lp;   // xrhip_ba_solve drops the landmark rows when no landmark is free
    d.nfree = 0;
    for (int f = 0; f < F; ++f) d.nfree += (P->frame_fix[f] & 3) != 3 ? 1 : 0;
    d.nffp = 0;
    for (int o = 0; o < M; ++o)
        d.nffp += (!(P->frame_fix[P->obs_tgt[o]] & XRHIP_FIX_POSE) && !(P->frame_fix[P->obs_ref[o]] & XRHIP_FIX_POSE)) ? 1 : 0;
    ix.imuf.assign(2 * F, -1);
    ix.priorf.assign(F, -1);
    for (int k = 0; k < NI; ++k) {
        if (ix.imuf[2 * P->imu_j[k]] >= 0 || ix.imuf[2 * P->imu_i[k] + 1] >= 0)
            return "xrhip_ba_solve: a frame may end at most one IMU factor and start at most one";
        ix.imuf[2 * P->imu_j[k]] = k;
        ix.imuf[2 * P->imu_i[k] + 1] = k;
    }
    for (int k = 0; k < NP; ++k) ix.priorf[P->prior_frames[k]] = k;
    ix.bias_ref.assign((size_t)6 * std::max(NI, 1), 0.0);
    for (int k = 0; k < NI; ++k)
        for (int i = 0; i < 6; ++i) ix.bias_ref[6 * k + i] = P->frame_state[16 * P->imu_i[k] + 10 + i];
    return nullptr;
}

// ---------------------------------------------------------------------------------------------- the layout
// Every buffer a solve addresses through BaPtrs, once: the member it feeds, its bytes as a function of BaDims `d`, and
//   IN  -- input arena (pinned host block, pulled to the device by kb_stage); third field: where its bytes come from
//          (P: the problem, ix: its StageIndex, ctl: the solve's initial BaCtl);
//   WS  -- device workspace;
//   LIN -- device workspace, a linearisation product: one of the buffers that exist twice under speculation (spec_set) and change
//          places when a speculation is taken (swap_lin_sets).  Marking it here is all it takes.
// Each arena is bumped in list order (bump256).  THE ORDER AND THE SIZES ARE FROZEN: device addresses feed cache and channel
// behaviour, so a buffer is added at the end of its arena's entries, and nothing here is reordered, merged or dropped to tidy up.
// The TinyArgs block follows the last IN entry (stage_layout), so BaCtl and TinyArgs end the input arena.
constexpr size_t D8 = sizeof(double);
#define XRHIP_BA_LAYOUT(IN, WS, LIN)                                                     \
    IN(state, D8 * 16 * d.F, P->frame_state)                                             \
    IN(fix, d.F, P->frame_fix)                                                           \
    IN(depth, D8 * d.L, P->inv_depth)                                                    \
    IN(lact, std::max(d.L, 1), ix.lact.data())                                           \
    IN(obs_tgt, sizeof(int) * d.M, P->obs_tgt)                                           \
    IN(obs_ref, sizeof(int) * d.M, P->obs_ref)                                           \
    IN(obs_lm, sizeof(int) * d.M, P->obs_lm)                                             \
    IN(obs_zt, D8 * 3 * d.M, P->obs_z_tgt)                                               \
    IN(obs_zr, D8 * 3 * d.M, P->obs_z_ref)                                               \
    IN(rot_tgt, sizeof(int) * d.MR, P->rot_tgt)                                          \
    IN(rot_ref, sizeof(int) * d.MR, P->rot_ref)                                          \
    IN(rot_zt, D8 * 3 * d.MR, P->rot_z_tgt)                                              \
    IN(rot_zr, D8 * 3 * d.MR, P->rot_z_ref)                                              \
    IN(imu_i, sizeof(int) * d.NI, P->imu_i)                                              \
    IN(imu_j, sizeof(int) * d.NI, P->imu_j)                                              \
    IN(imu_data, D8 * XRHIP_IMU_DIM * d.NI, P->imu_data)                                 \
    IN(bias_ref, D8 * 6 * d.NI, ix.bias_ref.data())                                      \
    IN(prior_frames, sizeof(int) * d.NP, P->prior_frames)                                \
    IN(pS, D8 * (size_t)d.np * d.np, P->prior_sqrt_info)                                 \
    IN(pinfo, D8 * d.np, P->prior_infovec)                                               \
    IN(plin, D8 * 16 * d.NP, P->prior_lin)                                               \
    IN(lm_start, sizeof(int) * (d.L + 1), ix.lm_start.data())                            \
    IN(lm_obs, sizeof(int) * d.M, ix.lm_obs.data())                                      \
    IN(pair_start, sizeof(int) * ((size_t)d.F * d.F + 1), ix.pair_start.data())          \
    IN(pair_items, sizeof(int) * 4 * d.M, ix.pair_items.data())                          \
    IN(rotf_start, sizeof(int) * (d.F + 1), ix.rotf_start.data())                        \
    IN(rotf_items, sizeof(int) * d.MR, ix.rotf_items.data())                             \
    IN(imuf, sizeof(int) * 2 * d.F, ix.imuf.data())                                      \
    IN(priorf, sizeof(int) * d.F, ix.priorf.data())                                      \
    IN(act_idx, sizeof(int) * (size_t)d.na, ix.act_idx.data())                           \
    IN(act_inv, sizeof(int) * (size_t)d.n, ix.act_inv.data())                            \
    IN(ctl, sizeof(BaCtl), &ctl)                                                         \
    WS(cand, D8 * 16 * d.F * TRY_B)                                                      \
    WS(depth_cand, D8 * d.L * TRY_B)                                                     \
    WS(pLam, D8 * (size_t)d.np * d.np)                                                   \
    WS(pc0, D8 * d.np)                                                                   \
    LIN(orec, D8 * OREC * d.M)                                                           \
    LIN(ocost, D8 * d.M)                                                                 \
    LIN(rrec, D8 * RREC * d.MR)                                                          \
    LIN(rcost, D8 * d.MR)                                                                \
    LIN(imu_r, D8 * 15 * d.NI)                                                           \
    LIN(imu_Ji, D8 * 225 * d.NI)                                                         \
    LIN(imu_Jj, D8 * 225 * d.NI)                                                         \
    LIN(imu_cost, D8 * d.NI)                                                             \
    LIN(pr, D8 * d.np)                                                                   \
    LIN(pt, D8 * d.np)                                                                   \
    LIN(pJq, D8 * 9 * d.NP)                                                              \
    LIN(pcost, D8 * (1 + (d.np + 15) / 16))                                              \
    LIN(Hpp, D8 * (size_t)d.n * d.n)                                                     \
    LIN(gp, D8 * d.n)                                                                    \
    LIN(hll, D8 * d.Lp)                                                                  \
    LIN(gl, D8 * d.Lp)                                                                   \
    LIN(Wt, D8 * (size_t)d.Lp * d.PF)                                                    \
    WS(sp, D8 * d.n)                                                                     \
    WS(sl, D8 * d.Lp)                                                                    \
    LIN(omega, D8 * d.Lp)                                                                \
    LIN(T, D8 * (size_t)d.PF * d.PF)                                                     \
    LIN(Sred, D8 * (size_t)d.n * d.n)                                                    \
    LIN(diagD, D8 * d.NV)                                                                \
    WS(grad, D8 * d.NV)                                                                  \
    WS(gn, D8 * d.NV)                                                                    \
    LIN(gs, D8 * d.NV)                                                                   \
    WS(step, D8 * d.NV)                                                                  \
    WS(delta, D8 * d.NV * TRY_B)                                                         \
    LIN(partial, D8 * (size_t)(aux_quad_blocks_n(d.n, std::max(d.L, 1)) + 8))            \
    LIN(wog, D8 * d.PF * WOG_CH)                                                         \
    WS(wide_part, D8 * WIDE_G * 4 * WIDE_B)                                              \
    LIN(Hv, D8 * 36 * (size_t)d.F * d.F * VIS_CH)                                        \
    LIN(gv, D8 * 6 * d.F * VIS_CH)
#define XRHIP_BA_SKIP(...)

struct StageLayout {
    size_t o_args = 0;        // the TinyArgs block, behind the last entry of the input arena
    size_t in_bytes = 0;      // input arena: what kb_stage copies
    size_t work_bytes = 0;    // device workspace
    size_t out_doubles = 0;   // pinned readback: states, depths
};
inline StageLayout stage_layout(const BaDims &d) {
    size_t in = 0, ws = 0;
#define XRHIP_IN(m, bytes, src) bump256(in, bytes);
#define XRHIP_WS(m, bytes) bump256(ws, bytes);
    XRHIP_BA_LAYOUT(XRHIP_IN, XRHIP_WS, XRHIP_WS)
#undef XRHIP_IN
#undef XRHIP_WS
    StageLayout l;
    l.o_args = bump256(in, sizeof(TinyArgs));
    l.in_bytes = in + 256;
    l.work_bytes = ws + 256;
    l.out_doubles = (size_t)16 * d.F + d.L + 8;
    return l;
}

template <class T> inline void set_at(gptr<T> &m, char *addr) { m = reinterpret_cast<T *>(addr); }

// The pointers of a solve from the two base addresses (the mailbox members host_ctl / host_out / host_seq are the caller's).
inline void stage_fill_ptrs(BaPtrs &p, const BaDims &d, char *in_dev, char *work) {
    size_t in = 0, ws = 0;
#define XRHIP_IN(m, bytes, src) set_at(p.m, in_dev + bump256(in, bytes));
#define XRHIP_WS(m, bytes) set_at(p.m, work + bump256(ws, bytes));
    XRHIP_BA_LAYOUT(XRHIP_IN, XRHIP_WS, XRHIP_WS)
#undef XRHIP_IN
#undef XRHIP_WS
}

// The input arena's content, written into its pinned host mirror (the TinyArgs block is the caller's: it holds device addresses).
inline void stage_copy_inputs(char *in_host, const BaDims &d, const xrhip_ba_problem *P, const StageIndex &ix, const BaCtl &ctl) {
    size_t in = 0;
#define XRHIP_IN(m, bytes, src)                                                \
    {                                                                          \
        const size_t b = bytes, off = bump256(in, b);                          \
        const void *s = src;                                                   \
        if (b && s) std::memcpy(in_host + off, s, b);                          \
    }
    XRHIP_BA_LAYOUT(XRHIP_IN, XRHIP_BA_SKIP, XRHIP_BA_SKIP)
#undef XRHIP_IN
}

// ---------------------------------------------------------------------------------------------- the second set (speculation)
// work_spec mirrors the workspace (work_cap bytes) and holds, behind it, the candidate's state / depth / control block.
inline size_t spec_extra_bytes(const BaDims &d) {
    return sizeof(double) * (16 * (size_t)d.F + (size_t)std::max(d.L, 1)) + sizeof(BaCtl) + 1024;
}
template <class T> inline void rebase(gptr<T> &m, const char *from, char *to) {
    m = reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(static_cast<T *>(m)) - reinterpret_cast<uintptr_t>(from) + reinterpret_cast<uintptr_t>(to));
}
inline BaPtrs spec_set(const BaPtrs &p, const BaDims &d, char *work, char *work_spec, size_t work_cap) {
    BaPtrs p2 = p;
#define XRHIP_LIN(m, bytes) rebase(p2.m, work, work_spec);
    XRHIP_BA_LAYOUT(XRHIP_BA_SKIP, XRHIP_BA_SKIP, XRHIP_LIN)
#undef XRHIP_LIN
    char *x = work_spec + ((work_cap + 255) & ~size_t(255));
    set_at(p2.state, x);
    set_at(p2.depth, x + sizeof(double) * 16 * (size_t)d.F);
    set_at(p2.ctl, x + ((sizeof(double) * (16 * (size_t)d.F + (size_t)std::max(d.L, 1)) + 255) & ~size_t(255)));
    return p2;
}
// The products of the linearisation chain change places; state / depth / ctl stay the minimiser's.
inline void swap_lin_sets(BaPtrs &p, BaPtrs &p2) {
#define XRHIP_LIN(m, bytes) std::swap(p.m, p2.m);
    XRHIP_BA_LAYOUT(XRHIP_BA_SKIP, XRHIP_BA_SKIP, XRHIP_LIN)
#undef XRHIP_LIN
}

// ---------------------------------------------------------------------------------------------- scratch layouts
// Offsets into one block each, bumped in member order; `bytes` is what the block must hold.  Frozen like the list above.
struct MargScratch {   // device (work2); N = 15 K unknowns, R = N - 15 of them stay
    size_t Hm, bm, T2, A, bp, B, V, si, iv, st, lam, sup, As, bs, Ss, ivs, bytes;
    size_t host_bytes;   // pinned readback: sqrt_info [R x R], infovec [R], the eight status words
};
inline MargScratch marg_scratch(int N, int R) {
    const size_t n = (size_t)N, r = (size_t)R;
    size_t w = 0;
    MargScratch m;
    m.Hm = bump256(w, D8 * n * n);
    m.bm = bump256(w, D8 * n);
    m.T2 = bump256(w, D8 * r * 15);
    m.A = bump256(w, D8 * r * r);
    m.bp = bump256(w, D8 * r);
    m.B = bump256(w, D8 * r * r);
    m.V = bump256(w, D8 * r * r);
    m.si = bump256(w, D8 * r * r);
    m.iv = bump256(w, D8 * r);
    m.st = bump256(w, sizeof(int) * 8);
    m.lam = bump256(w, D8 * 2);
    m.sup = bump256(w, sizeof(int) * r);
    m.As = bump256(w, D8 * r * r);
    m.bs = bump256(w, D8 * r);
    m.Ss = bump256(w, D8 * r * r);
    m.ivs = bump256(w, D8 * r);
    m.bytes = w + 256;
    m.host_bytes = D8 * (r * r + r) + 64 + sizeof(int) * 8;
    return m;
}

struct CovScratch {   // device (cov_dev)
    size_t st, A, Li, ds, cols, B, Sig, out, var, bytes;
};
// n16: the reduced system's order padded to 16, nt = n16 / 16; groups: right-hand-side groups of 16 columns in B; full: the whole
// inverse is kept (Sig; an 8-byte stand-in otherwise); L: landmarks
inline CovScratch cov_scratch(int n16, int nt, int n_sel, int groups, bool full, int L) {
    size_t w = 0;
    CovScratch s;
    s.st = bump256(w, sizeof(CovStatus));
    s.A = bump256(w, D8 * (size_t)n16 * n16);
    s.Li = bump256(w, D8 * 256 * (size_t)nt);
    s.ds = bump256(w, D8 * n16);
    s.cols = bump256(w, sizeof(int) * 16 * (size_t)(n_sel + nt));
    s.B = bump256(w, D8 * 16 * (size_t)n16 * std::max(groups, 1));
    s.Sig = bump256(w, full ? D8 * (size_t)n16 * n16 : 8);
    s.out = bump256(w, D8 * 225 * (size_t)std::max(n_sel, 1));
    s.var = bump256(w, D8 * std::max(L, 1));
    s.bytes = w + 256;
    return s;
}

struct PreintScratch {   // pinned host (h_stage), addressed by the kernel over the host link
    size_t jobs, smp, noise, out, st, bytes;
};
inline PreintScratch preint_scratch(int n_jobs, int total_samples) {
    const size_t b_out = D8 * XRHIP_IMU_DIM * (size_t)n_jobs, b_st = 2 * sizeof(int) * n_jobs;   // status words, then the early-delta words
    size_t w = 0;
    PreintScratch s;
    s.jobs = bump256(w, sizeof(PreintJob) * n_jobs);
    s.smp = bump256(w, D8 * 7 * (size_t)total_samples);
    s.noise = bump256(w, D8 * 36);
    s.out = bump256(w, b_out + b_st);
    s.st = s.out + b_out;   // (the status words follow the results directly)
    s.bytes = w + 256;
    return s;
}

// The marginalisation's linearisation as a BA problem: every block free, no iteration.  state / fix / depth / lfix are the caller's
// and receive the copies the problem points at (they must outlive its staging).
inline xrhip_ba_problem marg_problem_view(const xrhip_marg_problem &M, std::vector<double> &state, std::vector<uint8_t> &fix,
                                          std::vector<double> &depth, std::vector<uint8_t> &lfix) {
    const int K = M.n_frames;
    state.assign(M.frame_state, M.frame_state + 16 * (size_t)K);
    fix.assign(K, 0);
    depth.assign(M.inv_depth, M.inv_depth + std::max(M.n_landmarks, 0));
    lfix.assign(std::max(M.n_landmarks, 1), 0);
    xrhip_ba_problem P;
    std::memset(&P, 0, sizeof(P));
    P.n_frames = K;
    P.frame_state = state.data();
    P.frame_fix = fix.data();
    std::memcpy(P.cam_q_bc, M.cam_q_bc, sizeof(P.cam_q_bc));
    std::memcpy(P.cam_p_bc, M.cam_p_bc, sizeof(P.cam_p_bc));
    std::memcpy(P.imu_q_bi, M.imu_q_bi, sizeof(P.imu_q_bi));
    std::memcpy(P.imu_p_bi, M.imu_p_bi, sizeof(P.imu_p_bi));
    std::memcpy(P.sqrt_inv_cov, M.sqrt_inv_cov, sizeof(P.sqrt_inv_cov));
    P.n_landmarks = M.n_landmarks;
    P.inv_depth = depth.data();
    P.landmark_fix = lfix.data();
    P.n_obs = M.n_obs;
    P.obs_tgt = M.obs_tgt;
    P.obs_ref = M.obs_ref;
    P.obs_lm = M.obs_lm;
    P.obs_z_tgt = M.obs_z_tgt;
    P.obs_z_ref = M.obs_z_ref;
    P.n_imu = M.n_imu;
    P.imu_i = M.imu_i;
    P.imu_j = M.imu_j;
    P.imu_data = M.imu_data;
    P.prior_n = M.prior_n;
    P.prior_frames = M.prior_frames;
    P.prior_sqrt_info = M.prior_sqrt_info;
    P.prior_infovec = M.prior_infovec;
    P.prior_lin = M.prior_lin;
    P.max_iterations = 0;
    return P;
}

}   // namespace xrhip
