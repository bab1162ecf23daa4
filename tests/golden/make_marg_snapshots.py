"""Generates tests/golden/marg_snapshots/*.npz: frozen marginalisation problems of the synthetic S1 / S2 / S3 streams -- what
Pipeline's marginalize_frame handed to xrhip_ba_marginalize -- with the CPU oracle's Lambda = S^T S, eta = S^T infovec, |infovec|
and support, asserted by tests/test_oracle_ba.py (the fixture is not stale) and tests/test_marg_shapes_gpu.py (the HIP path on
exactly the problems the pipeline produces).

    python tests/golden/make_marg_snapshots.py        # needs oracle/_build (make -C oracle); no GPU

The streams and the way they run are those of make_ba_snapshots.py (the CPU reference pipeline with XRSLAM_AMD_DUMP_BA set).  Kept
per stream: the first marginalisation (gauge prior: rank deficient, the eigen path), the last one (steady state, the window full)
and the one with the fewest landmarks (among those in between, where that is the first one itself).  The expected Lambda is stored as its upper triangle over the support."""
import glob
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ba_oracle as bo  # noqa: E402
from tests import ba_snapshots as snap  # noqa: E402
from tests import marg_metric as mm  # noqa: E402
from tests.golden.make_ba_snapshots import CFG, ORACLE_LIB, STREAMS  # noqa: E402
from xrslam_amd.harness import runner, scene  # noqa: E402

LIMIT = 480 * 1024      # the largest committed solve snapshot is 451 KB


def pack(d):
    md = snap.to_marg_problem(d)
    si, iv, _lin = bo.marginalize(md)
    lam, eta = mm.invariants(si, iv)
    sup = mm.support(lam)
    arrays = {k: d[k] for k in snap.MARG_FIELDS}
    arrays.update(exp_support=sup.astype(np.int32), exp_lam_upper=lam[np.ix_(sup, sup)][np.triu_indices(len(sup))], exp_eta=eta,
                  exp_iv_norm=np.float64(np.linalg.norm(iv)), exp_size=np.int32(len(lam)))
    return arrays, len(sup)


def main():
    out_dir = snap.MARG_DIR
    os.makedirs(out_dir, exist_ok=True)
    for name, cfg in STREAMS.items():
        tmp = tempfile.mkdtemp(prefix="xrmg_")
        os.environ["XRSLAM_AMD_DUMP_BA"] = tmp
        seq = scene.make_sequence(n_frames=cfg["n"], **cfg["kw"])
        s = runner.Session(ORACLE_LIB, seq, slam_yaml=os.path.join(CFG, cfg["slam"]), sensor_yaml=os.path.join(CFG, cfg["sensor"]))
        while s.step():
            assert not s.error(), s.error()
        s.flush()
        s.close()
        del os.environ["XRSLAM_AMD_DUMP_BA"]
        files = sorted(glob.glob(os.path.join(tmp, "marg_*.xrmg")))
        probs = [snap.read_xrmg(f) for f in files]
        print("%s: %d marginalisations dumped" % (name, len(files)))
        fewest = min(range(len(probs)), key=lambda i: (len(probs[i]["inv_depth"]), i))
        if fewest in (0, len(probs) - 1):      # the map is smallest at the first marginalisation: the fewest among those in between
            print("  fewest landmarks overall: marginalisation %d (L=%d), already kept" % (fewest, len(probs[fewest]["inv_depth"])))
            fewest = min(range(1, len(probs) - 1), key=lambda i: (len(probs[i]["inv_depth"]), i))
        picks = {"first": 0, "steady": len(probs) - 1, "fewest": fewest}
        for kind, i in picks.items():
            d = probs[i]
            arrays, nsup = pack(d)
            path = os.path.join(out_dir, "%s_%s.npz" % (name, kind))
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            print("  %-7s %s  F=%d NP=%d NI=%d L=%d M=%d  support %d of %d, %d KB%s"
                  % (kind, os.path.basename(files[i]), len(d["frame_state"]), len(d["prior_frames"]), len(d["imu_i"]),
                     len(d["inv_depth"]), len(d["obs_tgt"]), nsup, 15 * (len(d["frame_state"]) - 1), size // 1024,
                     "  -- over the limit, dropped" if size > LIMIT else ""))
            if size > LIMIT:
                os.remove(path)
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
