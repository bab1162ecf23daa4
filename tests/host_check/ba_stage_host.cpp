// Host-side access to the staging of a bundle-adjustment problem (xrslam_amd/csrc/ba_stage.hpp) for tests/test_ba_stage_host.py: the
// problem goes in as plain arrays; the counted sizes, the gather tables, the pointer sets (as raw 8-byte slots of BaPtrs, with the
// slot of every listed member) and the effect of the exchange come back as integers.  -DBA_STAGE_HOST_MAIN: a stand-alone program
// that stages four small problems into exactly sized heap blocks, for a run under the sanitizers.
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

int main() {
    const int shapes[4][6] = {{1, 0, 0, 0, 0, 0}, {2, 1, 1, 0, 0, 0}, {3, 17, 40, 3, 2, 2}, {13, 100, 700, 0, 12, 1}};
    for (const auto &s : shapes)
        if (stage_one(s[0], s[1], s[2], s[3], s[4], s[5])) {
            std::printf("ba_stage_host: shape F=%d L=%d M=%d failed\n", s[0], s[1], s[2]);
            return 1;
        }
    std::printf("ba_stage_host OK\n");
    return 0;
}
#endif
