"""The staging of a bundle-adjustment problem (xrslam_amd/csrc/ba_stage.hpp) compiled for the host with hipcc, no GPU: the gather
tables, the device layout of both arenas, the second pointer set of a speculative linearisation and the exchange of the two sets.

Device addresses feed cache and channel behaviour, so the layout is frozen: LAYOUT below is the put / carve sequence of stage_problem
as it stood before the layout moved into one table, transcribed once -- order, arena and size formula of every buffer -- and SPEC_SET
the members that the solve re-based into the second workspace and exchanged when a speculation was taken.  Every expected value here
comes from these literals and from arithmetic in this file, not from a second call of the code under test.

The same holds for the three scratch layouts that are not a staged problem's -- the marginalisation's, the covariance's and the
pre-integration staging block's (MARG_SCRATCH, COV_SCRATCH, PREINT_SCRATCH below) -- and marg_problem_view is checked field by field."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "ba_stage_host.cpp")
OUT = os.path.join(ROOT, "tests", "host_check", "_build", "libba_stage_host.so")
CSRC = os.path.join(ROOT, "xrslam_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

OREC, RREC, TRY_B, WIDE_G, WIDE_B, VIS_CH, WOG_CH = 28, 8, 4, 64, 8, 8, 8
IMU_DIM = int(re.search(r"#define XRHIP_IMU_DIM (\d+)", open(os.path.join(ROOT, "include", "xrslam_hip.h")).read()).group(1))


def aux_quad_blocks_n(n, L):
    return (n + 15) // 16 + (L + 31) // 32


# (BaPtrs member, arena, bytes): F L M MR NI NP as given; n = 15 F, PF = 6 F padded to 16, Lp = L padded to 16 (at least 16),
# np = 15 NP, NV = n + L, na = free frame dofs; CTL / ARGS = sizeof(BaCtl) / sizeof(TinyArgs)
LAYOUT = [
    ("state", "in", lambda d: 8 * 16 * d.F),
    ("fix", "in", lambda d: d.F),
    ("depth", "in", lambda d: 8 * d.L),
    ("lact", "in", lambda d: max(d.L, 1)),
    ("obs_tgt", "in", lambda d: 4 * d.M),
    ("obs_ref", "in", lambda d: 4 * d.M),
    ("obs_lm", "in", lambda d: 4 * d.M),
    ("obs_zt", "in", lambda d: 8 * 3 * d.M),
    ("obs_zr", "in", lambda d: 8 * 3 * d.M),
    ("rot_tgt", "in", lambda d: 4 * d.MR),
    ("rot_ref", "in", lambda d: 4 * d.MR),
    ("rot_zt", "in", lambda d: 8 * 3 * d.MR),
    ("rot_zr", "in", lambda d: 8 * 3 * d.MR),
    ("imu_i", "in", lambda d: 4 * d.NI),
    ("imu_j", "in", lambda d: 4 * d.NI),
    ("imu_data", "in", lambda d: 8 * IMU_DIM * d.NI),
    ("bias_ref", "in", lambda d: 8 * 6 * d.NI),
    ("prior_frames", "in", lambda d: 4 * d.NP),
    ("pS", "in", lambda d: 8 * d.np * d.np),
    ("pinfo", "in", lambda d: 8 * d.np),
    ("plin", "in", lambda d: 8 * 16 * d.NP),
    ("lm_start", "in", lambda d: 4 * (d.L + 1)),
    ("lm_obs", "in", lambda d: 4 * d.M),
    ("pair_start", "in", lambda d: 4 * (d.F * d.F + 1)),
    ("pair_items", "in", lambda d: 4 * 4 * d.M),
    ("rotf_start", "in", lambda d: 4 * (d.F + 1)),
    ("rotf_items", "in", lambda d: 4 * d.MR),
    ("imuf", "in", lambda d: 4 * 2 * d.F),
    ("priorf", "in", lambda d: 4 * d.F),
    ("act_idx", "in", lambda d: 4 * d.na),
    ("act_inv", "in", lambda d: 4 * 15 * d.F),
    ("ctl", "in", lambda d: d.CTL),
    ("<TinyArgs>", "in", lambda d: d.ARGS),
    ("cand", "ws", lambda d: 8 * 16 * d.F * TRY_B),
    ("depth_cand", "ws", lambda d: 8 * d.L * TRY_B),
    ("pLam", "ws", lambda d: 8 * d.np * d.np),
    ("pc0", "ws", lambda d: 8 * d.np),
    ("orec", "ws", lambda d: 8 * OREC * d.M),
    ("ocost", "ws", lambda d: 8 * d.M),
    ("rrec", "ws", lambda d: 8 * RREC * d.MR),
    ("rcost", "ws", lambda d: 8 * d.MR),
    ("imu_r", "ws", lambda d: 8 * 15 * d.NI),
    ("imu_Ji", "ws", lambda d: 8 * 225 * d.NI),
    ("imu_Jj", "ws", lambda d: 8 * 225 * d.NI),
    ("imu_cost", "ws", lambda d: 8 * d.NI),
    ("pr", "ws", lambda d: 8 * d.np),
    ("pt", "ws", lambda d: 8 * d.np),
    ("pJq", "ws", lambda d: 8 * 9 * d.NP),
    ("pcost", "ws", lambda d: 8 * (1 + (d.np + 15) // 16)),
    ("Hpp", "ws", lambda d: 8 * d.n * d.n),
    ("gp", "ws", lambda d: 8 * d.n),
    ("hll", "ws", lambda d: 8 * d.Lp),
    ("gl", "ws", lambda d: 8 * d.Lp),
    ("Wt", "ws", lambda d: 8 * d.Lp * d.PF),
    ("sp", "ws", lambda d: 8 * d.n),
    ("sl", "ws", lambda d: 8 * d.Lp),
    ("omega", "ws", lambda d: 8 * d.Lp),
    ("T", "ws", lambda d: 8 * d.PF * d.PF),
    ("Sred", "ws", lambda d: 8 * d.n * d.n),
    ("diagD", "ws", lambda d: 8 * d.NV),
    ("grad", "ws", lambda d: 8 * d.NV),
    ("gn", "ws", lambda d: 8 * d.NV),
    ("gs", "ws", lambda d: 8 * d.NV),
    ("step", "ws", lambda d: 8 * d.NV),
    ("delta", "ws", lambda d: 8 * d.NV * TRY_B),
    ("partial", "ws", lambda d: 8 * (aux_quad_blocks_n(d.n, max(d.L, 1)) + 8)),
    ("wog", "ws", lambda d: 8 * d.PF * WOG_CH),
    ("wide_part", "ws", lambda d: 8 * WIDE_G * 4 * WIDE_B),
    ("Hv", "ws", lambda d: 8 * 36 * d.F * d.F * VIS_CH),
    ("gv", "ws", lambda d: 8 * 6 * d.F * VIS_CH),
]
# the linearisation products: double-buffered under speculation
SPEC_SET = ["orec", "ocost", "rrec", "rcost", "imu_r", "imu_Ji", "imu_Jj", "imu_cost", "pr", "pt", "pJq", "pcost", "hll", "gl", "Wt", "Hv",
            "gv", "Hpp", "gp", "diagD", "gs", "omega", "T", "Sred", "partial", "wog"]
assert len(SPEC_SET) == len(set(SPEC_SET)) == 26

# F, L, M, MR, NI, NP: nothing but a frame; one of each visual kind; sizes that are no multiple of 16; a refine_window
SHAPES = {"frame_only": (1, 0, 0, 0, 0, 0), "one_obs": (2, 1, 1, 0, 0, 0), "odd": (3, 17, 40, 3, 2, 2), "window": (13, 100, 700, 0, 12, 1)}


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("ba_stage.hpp", "ba_plan.hpp", "ba_chain.hip.h", "ba_kernels.hip.h", "dense_lds.hip.h", "cov_kernels.hip.h",
                                                       "marg_kernels.hip.h")]
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", SRC, "-o", OUT])
    return C.CDLL(OUT)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def round_robin(F, L, M, MR, NI, NP):
    """a problem of the given sizes with every block free: factor o names frames o, o + 1 (mod F) and landmark o (mod L)"""
    o, r = np.arange(M), np.arange(MR)
    return dict(F=F, L=L, frame_fix=np.zeros(F, np.uint8), landmark_fix=np.zeros(L, np.uint8), obs_tgt=_i32(o % F), obs_ref=_i32((o + 1) % F),
                obs_lm=_i32(o % max(L, 1)), rot_tgt=_i32(r % F), imu_i=_i32(np.arange(NI)), imu_j=_i32(np.arange(NI) + 1),
                prior_frames=_i32(np.arange(NP)), frame_state=np.zeros((F, 16)))


class Dims:
    pass


def build(hc, pb):
    """-> (0 / 1, Dims or the refusal's text)"""
    dims, why = np.zeros(16, np.int32), C.create_string_buffer(128)
    fs = np.ascontiguousarray(pb["frame_state"], np.float64)
    rc = hc.hc_stage_build(pb["F"], pb["L"], len(pb["obs_tgt"]), len(pb["rot_tgt"]), len(pb["imu_i"]), len(pb["prior_frames"]), _ptr(fs),
                           _ptr(pb["frame_fix"]), _ptr(pb["landmark_fix"]), _ptr(pb["obs_tgt"]), _ptr(pb["obs_ref"]), _ptr(pb["obs_lm"]),
                           _ptr(pb["rot_tgt"]), _ptr(pb["imu_i"]), _ptr(pb["imu_j"]), _ptr(pb["prior_frames"]), _ptr(dims), why)
    if rc:
        return rc, why.value.decode()
    d = Dims()
    for k, v in zip("F n PF L Lp M MR NI NP np NV na nla lm_rows nfree nffp".split(), dims):
        setattr(d, k, int(v))
    sizes = np.zeros(3, np.int64)
    hc.hc_stage_sizes(_ptr(sizes))
    d.CTL, d.ARGS, d.SLOTS = (int(v) for v in sizes)
    return 0, d


def table(hc, name):
    n = hc.hc_stage_table(name.encode(), None, 0)
    assert n >= 0, name
    out = np.zeros(n)
    hc.hc_stage_table(name.encode(), _ptr(out), n)
    return out if name == "bias_ref" else [int(v) for v in out]


def entries(hc):
    """the table as the header lists it: [(member, slot in BaPtrs, arena, is a linearisation product)]"""
    buf = C.create_string_buffer(8192)
    assert hc.hc_stage_entries(buf, len(buf)) > 0
    return [(m, int(s), a, int(lin)) for m, s, a, lin in (ln.split() for ln in buf.value.decode().splitlines())]


IN_DEV, WORK, WORK_SPEC, BLANK = 0x10000000, 0x20000000, 0x30000000, 0x7777777700


def layout(hc, d, work_cap):
    tot, p, p2 = np.zeros(4, np.uint64), np.zeros(d.SLOTS, np.uint64), np.zeros(d.SLOTS, np.uint64)
    u64 = C.c_ulonglong
    hc.hc_stage_layout(u64(IN_DEV), u64(WORK), u64(WORK_SPEC), u64(work_cap), u64(BLANK), _ptr(tot), _ptr(p), _ptr(p2))
    return [int(v) for v in tot], [int(v) for v in p], [int(v) for v in p2]


def bump(used, nbytes):
    off = (used + 255) // 256 * 256
    return off, off + max(nbytes, 8)


def expected_offsets(d):
    """-> {member: (arena, offset, span)}, in_bytes, work_bytes from LAYOUT alone"""
    used, out = {"in": 0, "ws": 0}, {}
    for name, arena, size in LAYOUT:
        off, used[arena] = bump(used[arena], size(d))
        out[name] = (arena, off, used[arena] - off)
    return out, used["in"] + 256, used["ws"] + 256


@pytest.mark.parametrize("shape", list(SHAPES))
def test_offsets_are_the_frozen_ones(hc, shape):
    rc, d = build(hc, round_robin(*SHAPES[shape]))
    assert rc == 0
    F, L, M, MR, NI, NP = SHAPES[shape]
    assert (d.F, d.L, d.M, d.MR, d.NI, d.NP, d.n, d.np, d.NV, d.na) == (F, L, M, MR, NI, NP, 15 * F, 15 * NP, 15 * F + L, 15 * F)
    assert (d.PF, d.Lp, d.lm_rows) == ((6 * F + 15) // 16 * 16, max(16, (L + 15) // 16 * 16), max(16, (L + 15) // 16 * 16))
    want, in_bytes, work_bytes = expected_offsets(d)
    (o_args, got_in, got_work, out_doubles), p, _ = layout(hc, d, work_cap=1 << 20)
    assert (got_in, got_work, out_doubles) == (in_bytes, work_bytes, 16 * F + L + 8)
    assert o_args == want["<TinyArgs>"][1]
    base = {"in": IN_DEV, "ws": WORK}
    ent = entries(hc)
    assert [(m, a) for m, _, a, _ in ent] == [(m, a) for m, a, _ in LAYOUT if m != "<TinyArgs>"]   # every buffer, once, in this order
    for m, slot, arena, _ in ent:
        assert p[slot] == base[arena] + want[m][1], m
    # structure: 256-aligned, at least 8 bytes each, disjoint within an arena and inside its total
    for arena, total in (("in", in_bytes), ("ws", work_bytes)):
        spans = sorted((off, off + span) for a, off, span in want.values() if a == arena)
        assert all(off % 256 == 0 and end - off >= 8 for off, end in spans)
        assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
        assert spans[-1][1] + 256 == total
    # BaCtl and TinyArgs end the input arena
    assert max(want, key=lambda m: (want[m][0] == "in", want[m][1])) == "<TinyArgs>" and want["ctl"][1] < o_args
    # the slots nobody listed (the mailbox in pinned host memory) are left alone
    listed = {slot for _, slot, _, _ in ent}
    assert len(listed) == len(ent) and all(p[s] == BLANK for s in range(d.SLOTS) if s not in listed)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_speculation_set_and_exchange(hc, shape):
    rc, d = build(hc, round_robin(*SHAPES[shape]))
    assert rc == 0
    work_cap = (1 << 20) + 8   # (not a multiple of 256: the candidate's blocks sit behind the next boundary)
    _, p, p2 = layout(hc, d, work_cap)
    slot = {m: s for m, s, _, _ in entries(hc)}
    assert sorted(m for m, _, _, lin in entries(hc) if lin) == sorted(SPEC_SET)
    x = WORK_SPEC + (work_cap + 255) // 256 * 256
    moved = {slot[m]: p[slot[m]] + (WORK_SPEC - WORK) for m in SPEC_SET}
    moved[slot["state"]] = x
    moved[slot["depth"]] = x + 8 * 16 * d.F
    moved[slot["ctl"]] = x + (8 * (16 * d.F + max(d.L, 1)) + 255) // 256 * 256
    assert len(moved) == 29
    assert p2 == [moved.get(s, p[s]) for s in range(d.SLOTS)]   # exactly these, by exactly this; nothing else
    # the exchange: the 26 change places, state / depth / ctl and everything else stay; twice is the identity
    a, b = np.array(p, np.uint64), np.array(p2, np.uint64)
    hc.hc_stage_swap(_ptr(a), _ptr(b))
    lin = {slot[m] for m in SPEC_SET}
    assert [int(v) for v in a] == [p2[s] if s in lin else p[s] for s in range(d.SLOTS)]
    assert [int(v) for v in b] == [p[s] if s in lin else p2[s] for s in range(d.SLOTS)]
    hc.hc_stage_swap(_ptr(a), _ptr(b))
    assert [int(v) for v in a] == p and [int(v) for v in b] == p2


def test_index_tables(hc):
    """F = 3, L = 17, M = 40, MR = 3, NI = 2, NP = 2 with hand-written factor lists."""
    F, L = 3, 17
    # observation o: landmark o % 16 (landmark 16 is never observed), frames (0,1) for o < 20, (1,2) for 20 <= o < 30, (2,0) from 30
    tgt = [0] * 20 + [1] * 10 + [2] * 10
    ref = [1] * 20 + [2] * 10 + [0] * 10
    lm = [o % 16 for o in range(40)]
    frame_fix = np.array([3, 0, 2], np.uint8)      # frame 0 constant, frame 1 free, frame 2: pose free, motion held
    landmark_fix = np.zeros(L, np.uint8)
    landmark_fix[[2, 5]] = 1
    state = np.arange(3 * 16, dtype=np.float64).reshape(3, 16)
    pb = dict(F=F, L=L, frame_fix=frame_fix, landmark_fix=landmark_fix, obs_tgt=_i32(tgt), obs_ref=_i32(ref), obs_lm=_i32(lm),
              rot_tgt=_i32([2, 0, 2]), imu_i=_i32([1, 0]), imu_j=_i32([2, 1]), prior_frames=_i32([2, 0]), frame_state=state)
    rc, d = build(hc, pb)
    assert rc == 0
    # free dofs: all 15 of frame 1, the 6 pose dofs of frame 2
    act = list(range(15, 30)) + list(range(30, 36))
    assert (d.na, d.nfree) == (21, 2) and table(hc, "act_idx") == act
    assert table(hc, "act_inv") == [-1] * 15 + list(range(15)) + list(range(15, 21)) + [-1] * 9
    # landmarks: 16 observed, two of them held, landmark 16 without an observation
    assert d.nla == 14
    assert table(hc, "lact") == [0 if l in (2, 5, 16) else 1 for l in range(17)]
    # both poses free: only the ten (1,2) observations
    assert d.nffp == 10
    # landmark l < 8 is seen by o = l, l + 16, l + 32; 8 <= l < 16 by o = l, l + 16; landmark 16 by none
    starts, obs = [0], []
    for l in range(17):
        mine = [o for o in range(40) if o % 16 == l and l < 16]
        obs += mine
        starts.append(len(obs))
    assert starts[:9] == [0, 3, 6, 9, 12, 15, 18, 21, 24] and starts[16:] == [40, 40]
    assert table(hc, "lm_start") == starts and table(hc, "lm_obs") == obs
    # frame pairs, row-major (a, b): a factor lists itself under (t,t) and (t,r) as target (role 0), under (r,r) and (r,t) as reference
    cells = {(a, b): [] for a in range(3) for b in range(3)}
    for o in range(40):
        t, r = tgt[o], ref[o]
        cells[(t, t)].append(2 * o)
        cells[(r, r)].append(2 * o + 1)
        cells[(t, r)].append(2 * o)
        cells[(r, t)].append(2 * o + 1)
    counts = [len(cells[(a, b)]) for a in range(3) for b in range(3)]
    assert counts == [30, 20, 10, 20, 30, 10, 10, 10, 20]      # (0,0): 20 as target + 10 as reference, ...
    assert table(hc, "pair_start") == [0] + list(np.cumsum(counts))
    assert table(hc, "pair_items") == [it for a in range(3) for b in range(3) for it in cells[(a, b)]]
    assert cells[(0, 2)] == [2 * o + 1 for o in range(30, 40)] and cells[(1, 0)] == [2 * o + 1 for o in range(20)]
    # rotation factors by target frame: factor 1 -> frame 0; factors 0, 2 -> frame 2
    assert table(hc, "rotf_start") == [0, 1, 1, 3] and table(hc, "rotf_items") == [1, 0, 2]
    # IMU factor 0 runs 1 -> 2, factor 1 runs 0 -> 1: [frame][ends here, starts here]
    assert table(hc, "imuf") == [-1, 1, 1, 0, 0, -1]
    assert table(hc, "priorf") == [1, -1, 0]
    # the biases of each factor's first frame
    np.testing.assert_array_equal(table(hc, "bias_ref"), np.concatenate([state[1, 10:16], state[0, 10:16]]))
    # a frame that ends two IMU factors is refused, and so is one that starts two
    for i, j in (([0, 1], [2, 2]), ([0, 0], [1, 2])):
        rc, why = build(hc, dict(pb, imu_i=_i32(i), imu_j=_i32(j)))
        assert rc == 1 and "a frame may end at most one IMU factor and start at most one" in why


def test_empty_problem_tables_keep_one_entry(hc):
    """F = 1 and nothing else: the tables a kernel is handed are never empty (the max(., 1) guards), the CSR starts are"""
    rc, d = build(hc, round_robin(*SHAPES["frame_only"]))
    assert rc == 0 and (d.na, d.nla, d.nfree, d.nffp) == (15, 0, 1, 0)
    assert table(hc, "lact") == [0] and table(hc, "lm_start") == [0] and table(hc, "lm_obs") == [0]
    assert table(hc, "pair_start") == [0, 0] and table(hc, "pair_items") == [0]
    assert table(hc, "rotf_start") == [0, 0] and table(hc, "rotf_items") == [0]
    assert table(hc, "imuf") == [-1, -1] and table(hc, "priorf") == [-1] and list(table(hc, "bias_ref")) == [0.0] * 6


# ---------------------------------------------------------------------------------------------- the three scratch layouts
# The bump256 sequences of marg_launch, xrhip_ba_covariance and preint_stage as they stood in ba_api.hip before the layouts moved
# into ba_stage.hpp, transcribed once: (name, bytes), in order.  COV_STATUS / PREINT_JOB = sizeof(CovStatus) / sizeof(PreintJob).
COV_STATUS, PREINT_JOB = 24, 72
MARG_SCRATCH = [
    ("Hm", lambda N, R: 8 * N * N), ("bm", lambda N, R: 8 * N), ("T2", lambda N, R: 8 * R * 15),
    ("A", lambda N, R: 8 * R * R), ("bp", lambda N, R: 8 * R), ("B", lambda N, R: 8 * R * R),
    ("V", lambda N, R: 8 * R * R), ("si", lambda N, R: 8 * R * R), ("iv", lambda N, R: 8 * R),
    ("st", lambda N, R: 4 * 8), ("lam", lambda N, R: 8 * 2), ("sup", lambda N, R: 4 * R),
    ("As", lambda N, R: 8 * R * R), ("bs", lambda N, R: 8 * R), ("Ss", lambda N, R: 8 * R * R), ("ivs", lambda N, R: 8 * R),
]
COV_SCRATCH = [
    ("st", lambda n16, nt, n_sel, groups, full, L: COV_STATUS),
    ("A", lambda n16, nt, n_sel, groups, full, L: 8 * n16 * n16),
    ("Li", lambda n16, nt, n_sel, groups, full, L: 8 * 256 * nt),
    ("ds", lambda n16, nt, n_sel, groups, full, L: 8 * n16),
    ("cols", lambda n16, nt, n_sel, groups, full, L: 4 * 16 * (n_sel + nt)),
    ("B", lambda n16, nt, n_sel, groups, full, L: 8 * 16 * n16 * max(groups, 1)),
    ("Sig", lambda n16, nt, n_sel, groups, full, L: 8 * n16 * n16 if full else 8),
    ("out", lambda n16, nt, n_sel, groups, full, L: 8 * 225 * max(n_sel, 1)),
    ("var", lambda n16, nt, n_sel, groups, full, L: 8 * max(L, 1)),
]
PREINT_SCRATCH = [
    ("jobs", lambda n_jobs, total: PREINT_JOB * n_jobs), ("smp", lambda n_jobs, total: 8 * 7 * total),
    ("noise", lambda n_jobs, total: 8 * 36),
    ("out", lambda n_jobs, total: 8 * IMU_DIM * n_jobs + 2 * 4 * n_jobs),   # the results, then the status and early-delta words
]
SEL_BATCH = 64   # selected frames per launch of kc_selected_inverse


def scratch_expected(table, *args):
    """-> ([offset of every entry], bytes the block must hold) from a table above alone"""
    used, offs = 0, []
    for _, size in table:
        off, used = bump(used, size(*args))
        offs.append(off)
    return offs, used + 256


def cov_args(na, n_sel, want_var, L, nla=1):
    """the arguments xrhip_ba_covariance lays its scratch out with, as it derived them before the layout moved"""
    full = bool(want_var and L > 0 and nla > 0)
    n16 = (na + 15) // 16 * 16
    nt = n16 // 16
    return n16, nt, n_sel, max(nt if full else 0, min(n_sel, SEL_BATCH)), full, L


def _scratch(hc, fn, n, *args):
    out = np.zeros(n, np.uint64)
    getattr(hc, fn)(*args, _ptr(out))
    return [int(v) for v in out]


def test_scratch_struct_sizes(hc):
    sizes = np.zeros(2, np.int64)
    hc.hc_scratch_sizes(_ptr(sizes))
    assert (int(sizes[0]), int(sizes[1])) == (COV_STATUS, PREINT_JOB)


@pytest.mark.parametrize("N,R", [(30, 15), (165, 150), (527, 512)])   # two frames; the pipeline's full window; the largest accepted
def test_marg_scratch_is_the_frozen_one(hc, N, R):
    offs, total = scratch_expected(MARG_SCRATCH, N, R)
    got = _scratch(hc, "hc_marg_scratch", 18, N, R)
    assert got[:16] == offs and got[16] == total
    assert got[17] == 8 * (R * R + R) + 64 + 4 * 8     # the pinned readback: sqrt_info, infovec, status words
    assert all(o % 256 == 0 for o in offs) and offs == sorted(set(offs)) and offs[0] == 0
    if (N, R) == (30, 15):
        assert total <= 1 << 20      # stays under the workspace's 1 MiB floor
    if (N, R) == (165, 150):
        assert total > 1 << 20       # ... and this one does not (tests/test_marg_shapes_gpu.py relies on both)


# na, selected frames, variances asked, landmarks: one free frame; a full window; the cap on both sides of SEL_BATCH
@pytest.mark.parametrize("L", (0, 100))
@pytest.mark.parametrize("na,n_sel,want_var", [(15, 1, False), (165, 11, True), (960, 64, True), (960, 65, True)])
def test_cov_scratch_is_the_frozen_one(hc, na, n_sel, want_var, L):
    args = cov_args(na, n_sel, want_var, L)
    n16, nt, _, groups, full, _ = args
    assert full == (want_var and L > 0)
    if na == 960:                  # 64 | 65 selected: the right-hand-side groups stop at SEL_BATCH, the column lists and blocks go on
        assert (n16, nt, groups) == (960, 60, 64)
    offs, total = scratch_expected(COV_SCRATCH, *args)
    got = _scratch(hc, "hc_cov_scratch", 10, n16, nt, n_sel, groups, int(full), L)
    assert got[:9] == offs and got[9] == total
    assert all(o % 256 == 0 for o in offs) and offs == sorted(set(offs)) and offs[0] == 0
    names = [n for n, _ in COV_SCRATCH]
    if not full:                                       # the 8-byte stand-in of the inverse takes one 256-byte slot
        assert offs[names.index("out")] - offs[names.index("Sig")] == 256


@pytest.mark.parametrize("n_jobs,total", [(1, 1), (12, 240)])
def test_preint_scratch_is_the_frozen_one(hc, n_jobs, total):
    offs, bytes_ = scratch_expected(PREINT_SCRATCH, n_jobs, total)
    got = _scratch(hc, "hc_preint_scratch", 6, n_jobs, total)
    assert got[:4] == offs and got[5] == bytes_
    assert got[4] == offs[3] + 8 * IMU_DIM * n_jobs     # the status words follow the results directly, inside the same bump


def test_marg_problem_view(hc):
    """Three frames, victim 1, a prior on frames 0 and 2, both IMU factors of the victim, three observations of two landmarks: every
    field of the BA problem the marginalisation is staged as.  Counts and the factor arrays are the marginalisation's own; frames and
    landmarks are copies with every block free; no rotation factor; no iteration."""
    from xrslam_amd import abi
    rng = np.random.default_rng(5)
    K, L, NP = 3, 2, 2
    md = abi.MargProblemData(
        rng.normal(size=(K, 16)), 1, rng.normal(size=7), rng.normal(size=7), [460.0, 457.0],
        dict(frames=[0, 2], sqrt_info=rng.normal(size=(15 * NP, 15 * NP)), infovec=rng.normal(size=15 * NP), lin=rng.normal(size=(NP, 16))),
        dict(i=[0, 1], j=[1, 2], data=rng.normal(size=(2, IMU_DIM))), [0.5, 0.25],
        dict(tgt=[1, 1, 2], ref=[0, 0, 1], lm=[0, 1, 1], z_tgt=rng.normal(size=(3, 3)), z_ref=rng.normal(size=(3, 3))))
    M = md.struct()
    ints, ptrs, ext = np.zeros(9, np.int32), np.zeros(32, np.uint64), np.zeros(16)
    state, fix, depth, lfix = np.full((K, 16), np.nan), np.full(K, 9, np.uint8), np.full(L, np.nan), np.full(L, 9, np.uint8)
    hc.hc_marg_view(C.byref(M), _ptr(ints), _ptr(ptrs), _ptr(ext), _ptr(state), _ptr(fix), _ptr(depth), _ptr(lfix))
    # n_frames n_landmarks n_obs n_rot n_imu prior_n max_iterations | landmark_fix, then frame_state / frame_fix / inv_depth are the copies
    assert list(ints) == [K, L, 3, 0, 2, NP, 0, 1, 1]
    mine = [md.obs_tgt, md.obs_ref, md.obs_lm, md.obs_z_tgt, md.obs_z_ref, md.imu_i, md.imu_j, md.imu_data, md.prior_frames,
            md.prior_sqrt_info, md.prior_infovec, md.prior_lin]
    got, want = [int(v) for v in ptrs[0::2]], [a.ctypes.data for a in mine] + [0] * 4      # the rotation factors' arrays: null
    assert got == want and [int(v) for v in ptrs[1::2]] == want
    np.testing.assert_array_equal(ext, np.concatenate([md.cam_ext[:4], md.cam_ext[4:7], md.imu_ext[:4], md.imu_ext[4:7], md.sqrt_inv_cov[:2]]))
    np.testing.assert_array_equal(state, md.frame_state)
    np.testing.assert_array_equal(depth, md.inv_depth)
    assert not fix.any() and not lfix.any()
    # no landmarks: the depth copy is empty, the constant flags keep one entry
    md0 = abi.MargProblemData(md.frame_state, 0, md.cam_ext, md.imu_ext, md.sqrt_inv_cov, None, None, np.zeros(0), None)
    M0 = md0.struct()
    lfix[:] = 9
    hc.hc_marg_view(C.byref(M0), _ptr(ints), _ptr(ptrs), _ptr(ext), _ptr(state), _ptr(fix), _ptr(depth), _ptr(lfix))
    assert list(ints) == [K, 0, 0, 0, 0, 0, 0, 1, 1] and list(lfix) == [0, 9]


def test_staging_under_sanitizers(tmp_path):
    """the same source as a stand-alone program: the four shapes staged into blocks of exactly the sizes the layout reports, the three
    scratch layouts touched at both ends of such blocks, and a marginalisation staged through marg_problem_view"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "ba_stage_host")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror"] + san +
                          ["-DBA_STAGE_HOST_MAIN", SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "ba_stage_host OK" in p.stdout, p.stdout + p.stderr
