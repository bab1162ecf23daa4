// Host-side access to the staging of a bundle-adjustment problem (xrslam_amd/csrc/ba_stage.hpp) for tests/test_ba_stage_host.py: the
// problem goes in as plain arrays; the counted sizes, the gather tables, the pointer sets (as raw 8-byte slots of BaPtrs, with the
// slot of every listed member), the effect of the exchange, the three scratch layouts and the marginalisation's view as a BA problem
// come back as integers.  -DBA_STAGE_HOST_MAIN: a stand-alone program that stages four small problems and a marginalisation and lays
// the scratch blocks out in exactly sized heap blocks, for a run under the sanitizers.
#include "../../xrslam_amd/csrc/ba_stage.hpp"

#include <cstddef>
#include <cstdio>
#include <string>

using namespace xrhip;

namespace {
constexpr int SLOTS = (int)(sizeof(BaPtrs) / 8);
static_assert(sizeof(BaPtrs) % 8 == 0, "BaPtrs is an array of pointers");

BaDims g_d;
StageIndex g_ix;

xrhip_ba_problem make_problem(int F, int L, int M, int MR, int NI, int NP, const double *frame_state, const unsigned char *frame_fix,
                              const unsigned char *landmark_fix, const int *obs_tgt, const int *obs_ref, const int *obs_lm, const int *rot_tgt,
                              const int *imu_i, const int *imu_j, const int *prior_frames) {
    xrhip_ba_problem P;
    std::memset(&P, 0, sizeof(P));
    P.n_frames = F;
    P.frame_state = const_cast<double *>(frame_state);
    P.frame_fix = frame_fix;
    P.n_landmarks = L;
    P.landmark_fix = landmark_fix;
    P.n_obs = M;
    P.obs_tgt = obs_tgt;
    P.obs_ref = obs_ref;
    P.obs_lm = obs_lm;
    P.n_rot = MR;
    P.rot_tgt = rot_tgt;
    P.n_imu = NI;
    P.imu_i = imu_i;
    P.imu_j = imu_j;
    P.prior_n = NP;
    P.prior_frames = prior_frames;
    return P;
}
}   // namespace

extern "C" {

// sizeof(BaCtl), sizeof(TinyArgs), 8-byte slots of BaPtrs
void hc_stage_sizes(long long *out3) {
    out3[0] = sizeof(BaCtl);
    out3[1] = sizeof(TinyArgs);
    out3[2] = SLOTS;
}

// one line per entry of the layout, in list order: "<member> <slot of the member in BaPtrs> <arena: in|ws> <1: linearisation product>"
int hc_stage_entries(char *buf, int cap) {
    std::string s;
#define HC_IN(m, bytes, src) s += std::string(#m) + " " + std::to_string(offsetof(BaPtrs, m) / 8) + " in 0\n";
#define HC_WS(m, bytes) s += std::string(#m) + " " + std::to_string(offsetof(BaPtrs, m) / 8) + " ws 0\n";
#define HC_LIN(m, bytes) s += std::string(#m) + " " + std::to_string(offsetof(BaPtrs, m) / 8) + " ws 1\n";
    XRHIP_BA_LAYOUT(HC_IN, HC_WS, HC_LIN)
#undef HC_IN
#undef HC_WS
#undef HC_LIN
    if ((int)s.size() + 1 > cap) return -1;
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

// index build; 0, or 1 when the problem is refused (the reason goes to `why`, 128 bytes).  dims16: F n PF L Lp M MR NI NP np NV na nla lm_rows nfree nffp
int hc_stage_build(int F, int L, int M, int MR, int NI, int NP, const double *frame_state, const unsigned char *frame_fix,
                   const unsigned char *landmark_fix, const int *obs_tgt, const int *obs_ref, const int *obs_lm, const int *rot_tgt,
                   const int *imu_i, const int *imu_j, const int *prior_frames, int *dims16, char *why) {
    const xrhip_ba_problem P = make_problem(F, L, M, MR, NI, NP, frame_state, frame_fix, landmark_fix, obs_tgt, obs_ref, obs_lm, rot_tgt, imu_i, imu_j, prior_frames);
    if (const char *w = stage_index(&P, 0, g_d, g_ix)) {
        std::snprintf(why, 128, "%s", w);
        return 1;
    }
    const BaDims &d = g_d;
    const int v[16] = {d.F, d.n, d.PF, d.L, d.Lp, d.M, d.MR, d.NI, d.NP, d.np, d.NV, d.na, d.nla, d.lm_rows, d.nfree, d.nffp};
    std::memcpy(dims16, v, sizeof(v));
    return 0;
}

// a table of the last build as doubles (every one holds small integers or copied biases): its length, or -1 for an unknown name
int hc_stage_table(const char *name, double *out, int cap) {
    const std::string n(name);
    auto give = [&](const auto &v) {
        for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = (double)v[i];
        return (int)v.size();
    };
    if (n == "lact") return give(g_ix.lact);
    if (n == "lm_start") return give(g_ix.lm_start);
    if (n == "lm_obs") return give(g_ix.lm_obs);
    if (n == "pair_start") return give(g_ix.pair_start);
    if (n == "pair_items") return give(g_ix.pair_items);
    if (n == "rotf_start") return give(g_ix.rotf_start);
    if (n == "rotf_items") return give(g_ix.rotf_items);
    if (n == "act_idx") return give(g_ix.act_idx);
    if (n == "act_inv") return give(g_ix.act_inv);
    if (n == "imuf") return give(g_ix.imuf);
    if (n == "priorf") return give(g_ix.priorf);
    if (n == "bias_ref") return give(g_ix.bias_ref);
    return -1;
}

// layout of the last build.  totals4: o_args, in_bytes, work_bytes, out_doubles; p / p2: the slots of the pointer set filled from the
// two base addresses (every slot preset to `blank`) and of the set spec_set makes from it
void hc_stage_layout(unsigned long long in_dev, unsigned long long work, unsigned long long work_spec, unsigned long long work_cap,
                     unsigned long long blank, unsigned long long *totals4, unsigned long long *p_slots, unsigned long long *p2_slots) {
    const StageLayout lay = stage_layout(g_d);
    totals4[0] = lay.o_args;
    totals4[1] = lay.in_bytes;
    totals4[2] = lay.work_bytes;
    totals4[3] = lay.out_doubles;
    for (int i = 0; i < SLOTS; ++i) p_slots[i] = blank;
    BaPtrs p;
    std::memcpy(&p, p_slots, sizeof(p));
    stage_fill_ptrs(p, g_d, reinterpret_cast<char *>(in_dev), reinterpret_cast<char *>(work));
    const BaPtrs p2 = spec_set(p, g_d, reinterpret_cast<char *>(work), reinterpret_cast<char *>(work_spec), (size_t)work_cap);
    std::memcpy(p_slots, &p, sizeof(p));
    std::memcpy(p2_slots, &p2, sizeof(p2));
}

void hc_stage_swap(unsigned long long *a_slots, unsigned long long *b_slots) {
    BaPtrs a, b;
    std::memcpy(&a, a_slots, sizeof(a));
    std::memcpy(&b, b_slots, sizeof(b));
    swap_lin_sets(a, b);
    std::memcpy(a_slots, &a, sizeof(a));
    std::memcpy(b_slots, &b, sizeof(b));
}

// the scratch layouts, members in declaration order.  marg: 16 offsets, bytes, host_bytes; cov: 9 offsets, bytes; preint: 5, bytes
void hc_marg_scratch(int N, int R, unsigned long long *out18) {
    const MargScratch m = marg_scratch(N, R);
    const size_t v[18] = {m.Hm, m.bm, m.T2, m.A, m.bp, m.B, m.V, m.si, m.iv, m.st, m.lam, m.sup, m.As, m.bs, m.Ss, m.ivs, m.bytes, m.host_bytes};
    for (int i = 0; i < 18; ++i) out18[i] = v[i];
}
void hc_cov_scratch(int n16, int nt, int n_sel, int groups, int full, int L, unsigned long long *out10) {
    const CovScratch s = cov_scratch(n16, nt, n_sel, groups, full != 0, L);
    const size_t v[10] = {s.st, s.A, s.Li, s.ds, s.cols, s.B, s.Sig, s.out, s.var, s.bytes};
    for (int i = 0; i < 10; ++i) out10[i] = v[i];
}
void hc_preint_scratch(int n_jobs, int total_samples, unsigned long long *out6) {
    const PreintScratch s = preint_scratch(n_jobs, total_samples);
    const size_t v[6] = {s.jobs, s.smp, s.noise, s.out, s.st, s.bytes};
    for (int i = 0; i < 6; ++i) out6[i] = v[i];
}
// sizeof(CovStatus), sizeof(PreintJob)
void hc_scratch_sizes(long long *out2) {
    out2[0] = sizeof(CovStatus);
    out2[1] = sizeof(PreintJob);
}

// marg_problem_view of *M.  ints9: n_frames n_landmarks n_obs n_rot n_imu prior_n max_iterations, 1 if landmark_fix is the lfix copy,
// 1 if frame_state / frame_fix / inv_depth are the other three copies; ptrs (32): every other pointer member followed by what it must
// equal (M's array, or null for the rotation factors); ext16: cam_q_bc cam_p_bc imu_q_bi imu_p_bi sqrt_inv_cov;
// state / fix / depth / lfix: the content of the copies (16 K, K, L, max(L, 1) entries)
void hc_marg_view(const xrhip_marg_problem *M, int *ints9, unsigned long long *ptrs, double *ext16, double *state, unsigned char *fix,
                  double *depth, unsigned char *lfix) {
    std::vector<double> vs, vd;
    std::vector<uint8_t> vf, vl;
    const xrhip_ba_problem P = marg_problem_view(*M, vs, vf, vd, vl);
    const int iv[9] = {P.n_frames, P.n_landmarks, P.n_obs, P.n_rot, P.n_imu, P.prior_n, P.max_iterations,
                       P.landmark_fix == vl.data(), P.inv_depth == vd.data() && P.frame_state == vs.data() && P.frame_fix == vf.data()};
    std::memcpy(ints9, iv, sizeof(iv));
    const void *pp[] = {P.obs_tgt, M->obs_tgt, P.obs_ref, M->obs_ref, P.obs_lm, M->obs_lm, P.obs_z_tgt, M->obs_z_tgt, P.obs_z_ref, M->obs_z_ref,
                        P.imu_i, M->imu_i, P.imu_j, M->imu_j, P.imu_data, M->imu_data, P.prior_frames, M->prior_frames,
                        P.prior_sqrt_info, M->prior_sqrt_info, P.prior_infovec, M->prior_infovec, P.prior_lin, M->prior_lin,
                        P.rot_tgt, nullptr, P.rot_ref, nullptr, P.rot_z_tgt, nullptr, P.rot_z_ref, nullptr};
    for (size_t i = 0; i < sizeof(pp) / sizeof(pp[0]); ++i) ptrs[i] = (unsigned long long)reinterpret_cast<uintptr_t>(pp[i]);
    std::memcpy(ext16, P.cam_q_bc, sizeof(double) * 4);
    std::memcpy(ext16 + 4, P.cam_p_bc, sizeof(double) * 3);
    std::memcpy(ext16 + 7, P.imu_q_bi, sizeof(double) * 4);
    std::memcpy(ext16 + 11, P.imu_p_bi, sizeof(double) * 3);
    std::memcpy(ext16 + 14, P.sqrt_inv_cov, sizeof(P.sqrt_inv_cov));
    std::memcpy(state, vs.data(), sizeof(double) * vs.size());
    std::memcpy(fix, vf.data(), vf.size());
    if (!vd.empty()) std::memcpy(depth, vd.data(), sizeof(double) * vd.size());
    std::memcpy(lfix, vl.data(), vl.size());
}

}   // extern "C"

#ifdef BA_STAGE_HOST_MAIN
// F, L, M, MR, NI, NP of the four shapes of tests/test_ba_stage_host.py; factor f of a kind names frames / landmarks round-robin
static int stage_one(int F, int L, int M, int MR, int NI, int NP) {
    std::vector<double> state((size_t)16 * F, 0.25), depth(L, 0.5), z((size_t)3 * std::max(M, MR), 1.0);
    std::vector<double> imu_data((size_t)XRHIP_IMU_DIM * NI, 0.0), pS((size_t)225 * NP * NP, 0.0), pinfo((size_t)15 * NP, 0.0), plin((size_t)16 * NP, 0.0);
    std::vector<unsigned char> fix(F, 0), lfix(L, 0);
    std::vector<int> tgt(M), ref(M), lm(M), rt(MR), rr(MR), ii(NI), ij(NI), pf(NP);
    for (int o = 0; o < M; ++o) {
        tgt[o] = o % F;
        ref[o] = (o + 1) % F;
        lm[o] = o % L;
    }
    for (int o = 0; o < MR; ++o) {
        rt[o] = o % F;
        rr[o] = (o + 1) % F;
    }
    for (int k = 0; k < NI; ++k) {
        ii[k] = k;
        ij[k] = k + 1;
    }
    for (int k = 0; k < NP; ++k) pf[k] = k;
    // empty arrays as null pointers, as a caller without such factors passes them
    auto ptr = [](auto &v) { return v.empty() ? nullptr : v.data(); };
    xrhip_ba_problem P = make_problem(F, L, M, MR, NI, NP, state.data(), fix.data(), ptr(lfix), ptr(tgt), ptr(ref), ptr(lm), ptr(rt), ptr(ii), ptr(ij), ptr(pf));
    P.inv_depth = ptr(depth);
    P.obs_z_tgt = P.obs_z_ref = M ? z.data() : nullptr;
    P.rot_ref = ptr(rr);
    P.rot_z_tgt = P.rot_z_ref = MR ? z.data() : nullptr;
    P.imu_data = ptr(imu_data);
    P.prior_sqrt_info = ptr(pS);
    P.prior_infovec = ptr(pinfo);
    P.prior_lin = ptr(plin);
    BaDims d;
    StageIndex ix;
    if (stage_index(&P, 0, d, ix)) return 1;
    const StageLayout lay = stage_layout(d);
    BaCtl ctl;
    std::memset(&ctl, 0, sizeof(ctl));
    // blocks of exactly the sizes the layout reports: a copy or a pointer past them is the sanitizer's to find
    std::vector<char> in_host(lay.in_bytes), in_dev(lay.in_bytes), work(lay.work_bytes), work_spec(lay.work_bytes + spec_extra_bytes(d));
    stage_copy_inputs(in_host.data(), d, &P, ix, ctl);
    Staged st{};
    st.d = d;
    stage_fill_ptrs(st.p, d, in_dev.data(), work.data());
    *reinterpret_cast<TinyArgs *>(in_host.data() + lay.o_args) = st;
    Staged st2 = st;
    st2.p = spec_set(st.p, d, work.data(), work_spec.data(), work.size());
    // the first and the last byte of every buffer, in both sets (64 doubles of wide_part and one control block are always there)
    static_cast<double *>(st.p.wide_part)[WIDE_G * 4 * WIDE_B - 1] = 1.0;
    static_cast<BaCtl *>(st2.p.ctl)->prof[31] = 1;
    static_cast<double *>(st2.p.state)[16 * F - 1] = 1.0;
    static_cast<double *>(st2.p.depth)[std::max(L, 1) - 1] = 1.0;
    static_cast<double *>(st2.p.gv)[6 * F * VIS_CH - 1] = 1.0;
    static_cast<double *>(st.p.gv)[6 * F * VIS_CH - 1] = 1.0;
    static_cast<double *>(st.p.Hpp)[(size_t)d.n * d.n - 1] = 1.0;
    static_cast<double *>(st2.p.Hpp)[(size_t)d.n * d.n - 1] = 1.0;
    swap_lin_sets(st.p, st2.p);
    static_cast<double *>(st.p.Sred)[(size_t)d.n * d.n - 1] = 2.0;
    static_cast<double *>(st2.p.Sred)[(size_t)d.n * d.n - 1] = 2.0;
    const BaCtl *staged_ctl = reinterpret_cast<const BaCtl *>(in_host.data() + (static_cast<char *>(static_cast<void *>(static_cast<BaCtl *>(st.p.ctl))) - in_dev.data()));
    return staged_ctl->iteration;   // 0: the control block went where BaPtrs::ctl says it is
}

// the scratch layouts in blocks of exactly the sizes they report: the first byte of every buffer and the last of the last one
static void touch(std::vector<char> &blk, std::initializer_list<size_t> offs, size_t last_byte) {
    for (size_t o : offs) blk[o] = 1;
    blk[last_byte] = 1;
}
static void scratch_all() {
    const int ms[3][2] = {{30, 15}, {165, 150}, {527, 512}};
    for (const auto &s : ms) {
        const MargScratch m = marg_scratch(s[0], s[1]);
        std::vector<char> blk(m.bytes);
        touch(blk, {m.Hm, m.bm, m.T2, m.A, m.bp, m.B, m.V, m.si, m.iv, m.st, m.lam, m.sup, m.As, m.bs, m.Ss, m.ivs}, m.ivs + D8 * s[1] - 1);
    }
    const int cs[4][6] = {{16, 1, 1, 1, 0, 0}, {176, 11, 11, 11, 1, 100}, {960, 60, 64, 64, 1, 100}, {960, 60, 65, 64, 0, 0}};
    for (const auto &s : cs) {
        const CovScratch c = cov_scratch(s[0], s[1], s[2], s[3], s[4] != 0, s[5]);
        std::vector<char> blk(c.bytes);
        touch(blk, {c.st, c.A, c.Li, c.ds, c.cols, c.B, c.Sig, c.out, c.var}, c.var + D8 * std::max(s[5], 1) - 1);
    }
    const int ps[2][2] = {{1, 1}, {12, 240}};
    for (const auto &s : ps) {
        const PreintScratch p = preint_scratch(s[0], s[1]);
        std::vector<char> blk(p.bytes);
        touch(blk, {p.jobs, p.smp, p.noise, p.out, p.st}, p.st + 2 * sizeof(int) * s[0] - 1);
    }
}

// a marginalisation (three frames, a prior on two, both IMU factors of the victim, three observations) staged through its view
static int marg_view_one() {
    const int K = 3, L = 2, M = 3, NI = 2, NP = 2;
    std::vector<double> state((size_t)16 * K, 0.25), depth(L, 0.5), z((size_t)3 * M, 1.0), imu_data((size_t)XRHIP_IMU_DIM * NI, 0.0);
    std::vector<double> pS((size_t)225 * NP * NP, 0.0), pinfo((size_t)15 * NP, 0.0), plin((size_t)16 * NP, 0.0);
    const int tgt[M] = {1, 1, 2}, ref[M] = {0, 0, 1}, lm[M] = {0, 1, 1}, ii[NI] = {0, 1}, ij[NI] = {1, 2}, pf[NP] = {0, 2};
    xrhip_marg_problem Mp;
    std::memset(&Mp, 0, sizeof(Mp));
    Mp.n_frames = K;
    Mp.victim = 1;
    Mp.frame_state = state.data();
    Mp.prior_n = NP;
    Mp.prior_frames = pf;
    Mp.prior_sqrt_info = pS.data();
    Mp.prior_infovec = pinfo.data();
    Mp.prior_lin = plin.data();
    Mp.n_imu = NI;
    Mp.imu_i = ii;
    Mp.imu_j = ij;
    Mp.imu_data = imu_data.data();
    Mp.n_landmarks = L;
    Mp.inv_depth = depth.data();
    Mp.n_obs = M;
    Mp.obs_tgt = tgt;
    Mp.obs_ref = ref;
    Mp.obs_lm = lm;
    Mp.obs_z_tgt = Mp.obs_z_ref = z.data();
    std::vector<double> vs, vd;
    std::vector<uint8_t> vf, vl;
    const xrhip_ba_problem P = marg_problem_view(Mp, vs, vf, vd, vl);
    BaDims d;
    StageIndex ix;
    if (stage_index(&P, 0, d, ix)) return 1;
    BaCtl ctl;
    std::memset(&ctl, 0, sizeof(ctl));
    std::vector<char> in_host(stage_layout(d).in_bytes);
    stage_copy_inputs(in_host.data(), d, &P, ix, ctl);
    return d.na == 15 * K && d.nla == L && P.max_iterations == 0 ? 0 : 1;
}

int main() {
    const int shapes[4][6] = {{1, 0, 0, 0, 0, 0}, {2, 1, 1, 0, 0, 0}, {3, 17, 40, 3, 2, 2}, {13, 100, 700, 0, 12, 1}};
    for (const auto &s : shapes)
        if (stage_one(s[0], s[1], s[2], s[3], s[4], s[5])) {
            std::printf("ba_stage_host: shape F=%d L=%d M=%d failed\n", s[0], s[1], s[2]);
            return 1;
        }
    scratch_all();
    if (marg_view_one()) {
        std::printf("ba_stage_host: marginalisation view failed\n");
        return 1;
    }
    std::printf("ba_stage_host OK\n");
    return 0;
}
#endif
