"""tests/cur_oracle.py against goldens made by the real reference (tests/golden/gen_golden_cur.py): the draws exactly, the
middle factor and the error to float64 round-off amplified by the conditioning of the case."""
import numpy as np
import pytest

import cur_cases as cc
import cur_oracle as co
from conftest import load_golden

PAIRS = [(name, kind) for name in sorted(cc.CUR_CASES) for kind in cc.KINDS]


@pytest.mark.parametrize("name,kind", PAIRS)
def test_oracle_reproduces_the_reference(name, kind):
    g = load_golden("%s_%s" % (kind, name))
    c = cc.case(name, kind)
    assert int(g["seed"]) == c["seed"] and int(g["rrank"]) == c["rrank"]
    for q in ("rid", "cid", "rcnt", "ccnt"):
        assert np.array_equal(np.asarray(c[q], dtype=np.float64), g[q].astype(np.float64)), q
    assert c["U"].shape == g["U"].shape == (len(c["cid"]), len(c["rid"]))
    # the same formula in the same precision: only the eigen-solver's and BLAS' round-off, amplified by the conditioning
    bound = (c["kappa_c"] + c["kappa_r"]) * 1e-12
    du = cc.rel_max(c["U"], g["U"])
    df = abs(c["ferr"] - float(g["ferr"])) / np.linalg.norm(c["data"].astype(np.float64))
    print("%s %s U %.3e (bound %.3e) ferr %.3e" % (kind, name, du, bound, df))
    assert du <= bound and df <= bound


@pytest.mark.parametrize("name", ["20x30", "300x40"])
def test_pinv_oracle_reproduces_the_reference(name):
    g = load_golden("pinv_" + name)
    rows, cols = (int(x) for x in g["A_shape"])
    A = np.random.RandomState(int(g["A_seed"])).rand(rows, cols).astype(np.float32).astype(np.float64)
    P = co.pinv(A)
    assert P.shape == g["P"].shape == (cols, rows)
    assert cc.rel_max(P, g["P"]) <= 1e-11
    assert cc.rel_max(P, np.linalg.pinv(A)) <= 1e-11


def test_cmdinit_merges_repeated_indices():
    rid, cid, rcnt, ccnt = co.cmdinit(np.int32([5, 2, 5, 9, 2, 5]), np.int32([0, 0, 3]))
    assert rid.tolist() == [2, 5, 9] and rcnt.tolist() == [2.0, 3.0, 1.0]
    assert cid.tolist() == [0, 3] and ccnt.tolist() == [2.0, 1.0]


def test_sample_raises_past_the_last_cumulative_value():
    np.random.seed(0)
    with pytest.raises(IndexError):
        co.sample(3, np.array([0.1, 0.1]))
