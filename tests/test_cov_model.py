"""CPU: the two evaluations of the covariance reference (tests/cov_model.py) agree to 1e-6 on every case the GPU tests use, so each
case's tolerance max(1e-9, 50 d_ref) tests something; a case too ill-conditioned for that is replaced, not loosened."""
import numpy as np
import pytest

from tests import cov_model as cm


@pytest.mark.parametrize("name", cm.CASES)
def test_reference_evaluations_agree(name):
    r = cm.reference(name)
    print("%s: na %d, free landmarks %d, cond %.3e, d_ref blocks %.3e, variances %.3e" % (
        name, r["na"], r["nla"], r["cond"], r["d_blocks"].max(), r["d_var"].max() if len(r["d_var"]) else 0.0))
    assert r["d_blocks"].max() < 1e-6
    if len(r["d_var"]):
        assert r["d_var"].max() < 1e-6
    for f in range(len(r["blocks"])):
        assert np.all(np.diag(r["blocks"][f]) >= 0)


def test_table_prints():
    t = cm.table()
    print(t)
    assert t.count("\n") == len(cm.CASES) + 1
