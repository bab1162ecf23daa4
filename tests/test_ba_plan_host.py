"""The solve plan of the bundle adjustment (xrslam_amd/csrc/ba_plan.hpp: plan_solve) compiled for the host with hipcc, pinned on
both sides of every boundary that the header of tests/test_ba_routes_gpu.py lists.  That test runs real problems on the GPU and
reads the plan back through xrhip_ba_debug_last_route; this one feeds bare sizes to the same function and needs no GPU.  The
expected values are literals taken from that table and from the LDS figures worked out by hand below, not a second call of the
code under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "ba_plan_host.cpp")
OUT = os.path.join(ROOT, "tests", "host_check", "_build", "libba_plan_host.so")
CSRC = os.path.join(ROOT, "xrslam_amd", "csrc")

NONE, TINY, CHAIN, SMALL_MID, MULTI = 0, 1, 2, 3, 4   # xrhip_ba_debug_last_route [0]
LDS = 150 * 1024


@pytest.fixture(scope="module")
def hc():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("ba_plan.hpp", "ba_chain.hip.h", "ba_kernels.hip.h", "dense_lds.hip.h")]
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", SRC, "-o", OUT])
    return C.CDLL(OUT)


def plan(hc, F, M, na, MR=0, NI=1, NP=0, nla=0, nfree=1, nffp=0, lds_limit=LDS):
    out = np.zeros(10, np.int64)
    hc.hc_ba_plan(F, M, MR, NI, NP, na, nla, nfree, nffp, lds_limit, out.ctypes.data_as(C.c_void_p))
    keys = ("route", "use_lds", "sred_tiled", "block", "wide_trials", "wide_first", "chain_lds", "chain_opts", "try_lds", "wide_lds")
    return dict(zip(keys, (int(v) for v in out)))


def head(pl):
    return tuple(pl[k] for k in ("route", "use_lds", "sred_tiled", "block", "wide_trials", "wide_first"))


def test_tiny_and_small_mid_boundaries(hc):
    # one free frame against held landmarks, with a prior (which keeps kb_chain out): kb_tiny up to 640 visual factors
    assert head(plan(hc, F=4, M=640, na=15, NP=1)) == (TINY, 2, 0, 0, 0, 0)
    assert head(plan(hc, F=4, M=600, MR=40, na=15, NP=1)) == (TINY, 2, 0, 0, 0, 0)
    assert head(plan(hc, F=4, M=600, MR=41, na=15, NP=1)) == (SMALL_MID, 2, 0, 512, 1, 0)
    assert head(plan(hc, F=4, M=641, na=15, NP=1)) == (SMALL_MID, 2, 0, 512, 1, 0)
    # kb_small_mid up to 16 unknowns, the wide launches beyond; never with a free landmark
    assert head(plan(hc, F=4, M=700, na=16, NP=1)) == (SMALL_MID, 2, 0, 512, 1, 0)
    assert head(plan(hc, F=4, M=700, na=17, NP=1)) == (MULTI, 2, 0, 512, 1, 0)
    assert head(plan(hc, F=4, M=700, na=30, NP=1, nfree=2)) == (MULTI, 2, 0, 512, 1, 0)
    assert head(plan(hc, F=4, M=700, na=15, NP=1, nla=1)) == (MULTI, 2, 0, 512, 1, 0)
    assert head(plan(hc, F=4, M=300, na=15, NP=1, nla=1)) == (MULTI, 2, 0, 256, 1, 0)


def test_chain_boundaries(hc):
    ok = dict(F=4, M=300, na=15, NI=1)   # localize_newframe-sized: the layout is a few KiB, both optional regions fit behind it
    pl = plan(hc, **ok)
    assert head(pl) == (CHAIN, -1, 0, 0, 0, 0) and pl["chain_opts"] == 3 and pl["try_lds"] == 0
    assert pl["chain_lds"] > 8 * (4 * 27 * 65 + 16 * 300)   # the two regions alone
    # refused by a prior, by a reprojection factor between two free poses, by a seventh free frame, by a ninth IMU factor
    assert plan(hc, **ok, NP=1)["route"] == TINY
    assert plan(hc, **ok, nffp=1)["route"] == TINY
    assert plan(hc, **dict(ok, na=90), nfree=6)["route"] == CHAIN
    assert plan(hc, **dict(ok, na=90), nfree=7)["route"] == MULTI
    assert plan(hc, **dict(ok, na=91), nfree=6)["route"] == MULTI
    assert plan(hc, **dict(ok, NI=8))["route"] == CHAIN
    assert plan(hc, **dict(ok, NI=9))["route"] == TINY
    assert plan(hc, **ok, nla=1)["route"] == MULTI
    # ... and by more than 1024 visual factors
    assert plan(hc, **dict(ok, M=1000), MR=24)["route"] == CHAIN
    assert plan(hc, **dict(ok, M=1000), MR=25)["route"] == SMALL_MID
    # ... and by LDS: six free frames with 977 factors need 144.0 KiB with five IMU factors (neither optional region fits behind
    # that) and 154.0 KiB with six
    pl = plan(hc, F=7, M=977, na=90, NI=5, nfree=6)
    assert head(pl) == (CHAIN, -1, 0, 0, 0, 0) and pl["chain_opts"] == 0
    assert round(pl["chain_lds"] / 1024, 1) == 144.0
    assert head(plan(hc, F=7, M=977, na=90, NI=6, nfree=6)) == (MULTI, 2, 0, 512, 1, 1)
    assert plan(hc, F=7, M=977, na=90, NI=6, nfree=6, lds_limit=160 * 1024)["route"] == CHAIN


def test_reduced_system_layouts(hc):
    # 150 KiB of LDS: tiled up to na = 165 (141.6 KiB; 167.3 at 180), packed at 180 (128.7 KiB; 150.8 at 195), from 195 in the
    # global buffer, tiled and in place, with only the 13 tile rows of L^-1 rhs in LDS
    win = dict(F=13, M=700, NI=12, NP=1, nla=100, nfree=13)
    pl = plan(hc, na=165, **win)
    assert head(pl) == (MULTI, 2, 0, 512, 1, 1) and round(pl["try_lds"] / 1024, 1) == 141.6
    pl = plan(hc, na=180, **win)
    assert head(pl) == (MULTI, 1, 0, 512, 1, 1) and round(pl["try_lds"] / 1024, 1) == 128.7
    pl = plan(hc, na=195, **win)
    assert head(pl) == (MULTI, 0, 1, 512, 1, 1)
    assert pl["try_lds"] == 8 * 4 * (15 + 15 * 12)   # the trials' TRY_B = 4 sets of prior / IMU residuals outweigh 8 * 16 * 13
    assert plan(hc, na=195, **dict(win, NP=0, NI=0))["try_lds"] == 8 * 16 * 13


def test_block_size_and_wide_boundaries(hc):
    win = dict(NI=4, NP=1, nla=50, nfree=5)
    # kb_solve_try<256> up to 64 unknowns and 640 visual factors
    assert head(plan(hc, F=8, M=300, na=64, **win)) == (MULTI, 2, 0, 256, 1, 0)
    assert head(plan(hc, F=8, M=300, na=65, **win)) == (MULTI, 2, 0, 512, 1, 0)
    assert head(plan(hc, F=8, M=600, MR=40, na=60, **win)) == (MULTI, 2, 0, 256, 1, 0)
    assert head(plan(hc, F=8, M=600, MR=41, na=60, **win)) == (MULTI, 2, 0, 512, 1, 0)
    # rejected trials on kb_trials_wide from 256 reprojection factors, up to 32 frames
    assert head(plan(hc, F=8, M=255, na=60, **win)) == (MULTI, 2, 0, 256, 0, 0)
    assert head(plan(hc, F=8, M=256, na=60, **win)) == (MULTI, 2, 0, 256, 1, 0)
    assert head(plan(hc, F=32, M=300, na=60, **win)) == (MULTI, 2, 0, 256, 1, 0)
    assert head(plan(hc, F=33, M=300, na=60, **win)) == (MULTI, 2, 0, 256, 0, 0)
    # ... the first trial too from 600 factors and 90 unknowns
    assert head(plan(hc, F=8, M=599, na=90, **win)) == (MULTI, 2, 0, 512, 1, 0)
    assert head(plan(hc, F=8, M=600, na=90, **win)) == (MULTI, 2, 0, 512, 1, 1)
    assert head(plan(hc, F=8, M=600, na=89, **win)) == (MULTI, 2, 0, 512, 1, 0)
    assert head(plan(hc, F=33, M=600, na=90, **win)) == (MULTI, 2, 0, 512, 0, 0)
    # kb_trials_wide: WIDE_B = 8 candidate states and priors, 4 x 8 rows of 257 partial sums
    assert plan(hc, F=8, M=600, na=90, **win)["wide_lds"] == 8 * (8 * (16 * 8 + 15) + 4 * 8 * 257)
