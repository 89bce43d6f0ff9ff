"""tests/cursl_oracle.py against goldens made by the real reference (tests/golden/gen_golden_cursl.py): the draws exactly, the
probabilities to the round-off of two float64 eigen-solvers amplified by the gap at the cut, the middle factor and the error
to float64 round-off amplified by the conditioning of the case."""
import numpy as np
import pytest

import cur_cases as cc
import cursl_cases as csc
import cursl_oracle as cso
from conftest import load_golden


@pytest.mark.parametrize("name", sorted(csc.CURSL_CASES))
def test_oracle_reproduces_the_reference(name):
    g = load_golden("cursl_" + name)
    c = csc.case(name)
    assert int(g["seed"]) == c["seed"] and int(g["rrank"]) == c["rrank"]
    for q in ("rid", "cid", "rcnt", "ccnt"):
        assert np.array_equal(np.asarray(c[q], dtype=np.float64), g[q].astype(np.float64)), q
    # numpy.linalg.svd here, eigh of the Gram matrix there: 1e-12 of round-off times the gap factor, on the cumulative sums
    for q in ("prow", "pcol"):
        assert c[q].ravel().shape == g[q].shape
        dp = float(np.max(np.abs(np.cumsum(c[q].ravel()) - np.cumsum(g[q]))))
        print("%s %s cumulative %.3e (bound %.3e)" % (name, q, dp, 1e-12 * c["g"]))
        assert dp <= 1e-12 * c["g"]
        assert abs(g[q].sum() - 1.0) <= 1e-12
    assert c["U"].shape == g["U"].shape == (len(c["cid"]), len(c["rid"]))
    bound = (c["kappa_c"] + c["kappa_r"]) * 1e-12
    du = cc.rel_max(c["U"], g["U"])
    df = abs(c["ferr"] - float(g["ferr"])) / np.linalg.norm(c["data"].astype(np.float64))
    print("%s U %.3e (bound %.3e) ferr %.3e" % (name, du, bound, df))
    assert du <= bound and df <= bound


def test_comp_prob_takes_the_vectors_above_the_cut():
    """k beyond the rank: all kept vectors, and the division by k cancels in the normalisation."""
    d = np.dot(np.random.RandomState(5).rand(6, 2), np.random.RandomState(6).rand(2, 9))       # rank 2
    lev, kk, lam = cso.leverage(d, 4)
    assert kk == 2 and int(np.sum(lam > cso.EPS)) == 2 and abs(lev.sum() - 2.0) <= 1e-12
    assert np.allclose(cso.comp_prob(d, 4), lev / 2.0, rtol=0, atol=1e-14)
    assert cso.gap_factor(lam, 2) == 1.0 and cso.gap_factor(lam, 1) > 1.0
    assert cso.ranks(d, 0) == (6, 9) and cso.ranks(d, 3) == (3, 3)
