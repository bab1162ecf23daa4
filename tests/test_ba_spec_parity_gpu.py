"""A window solve with and without the speculative linearisation gives the same bits.

DESIGN.md: the linearisation queued at the first candidate beside the trials (second stream, second set of linearisation buffers,
csrc/ba_stage.hpp: spec_set / swap_lin_sets) "is the one the round would have computed".  A linearisation product that is carved but
left out of the second set, or out of the exchange, makes a taken speculation read one buffer from the wrong set -- which only a solve
that TAKES a speculation shows.  The frozen window problem of the S1 stream does; XRHIP_NO_SPEC is read once per process, so each side
is a fresh child."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import ba_snapshots
from xrslam_amd import ba
pd = {name: pd for name, pd, _ in ba_snapshots.load_all()}["s1_window"].copy()
ctx = ba.BaContext()
sm = ctx.solve(pd)
print("route", ctx.debug_last_route())
print("summary", sm.iterations, sm.successful_steps, sm.termination, float(sm.initial_cost).hex(), float(sm.final_cost).hex())
print("states", np.ascontiguousarray(pd.frame_state, np.float64).tobytes().hex())
print("depths", np.ascontiguousarray(pd.inv_depth, np.float64).tobytes().hex())
ctx.close()
"""
TAKEN = re.compile(r"speculative linearisations: (\d+) launched, (\d+) taken")


def _child(no_spec):
    env = {k: v for k, v in os.environ.items() if k != "XRHIP_NO_SPEC"}
    env["XRHIP_HOSTPROF"] = "1"   # xrhip_ba_destroy then reports how many speculations the context launched and took
    if no_spec:
        env["XRHIP_NO_SPEC"] = "1"
    return subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)


def test_window_solve_is_bit_identical_with_and_without_speculation():
    a = _child(no_spec=False)
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-2000:]   # (the second child is not started behind a failed first)
    b = _child(no_spec=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    m = TAKEN.search(a.stderr)
    assert m and int(m.group(2)) >= 1, a.stderr[-2000:]   # the problem is one that takes a speculation ...
    assert not TAKEN.search(b.stderr), b.stderr[-2000:]   # ... and the switch turns it off
    la, lb = a.stdout.splitlines(), b.stdout.splitlines()
    assert [ln.split()[0] for ln in la] == ["route", "summary", "states", "depths"]
    assert la == lb
