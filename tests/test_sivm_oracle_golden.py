"""tests/sivm_oracle.py against the goldens made by the real reference (tests/golden/gen_golden_sivm.py): select and W
exactly, H and ferr to 1e-10; every golden H satisfies the KKT conditions of its columns' problems.  No GPU."""
import numpy as np
import pytest

import sivm_cases as sc
import sivm_oracle as so
from conftest import load_golden

GOLDENS = ["sivm_doc_2x3_k2", "sivm_doc_userw", "sivm_37x29_k5", "sivm_29x300_k6_l2", "sivm_29x300_k6_l1",
           "sivm_29x300_k6_cosine", "sivm_29x300_k6_origin"]


def golden_v(g):
    if "case" in g:
        c = sc.CASES[str(g["case"])]
        return sc.planted(*c[:6], special=c[8])[0]
    return g["V"]


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_reproduces_golden(name):
    g = load_golden(name)
    V = golden_v(g).astype(np.float64)
    if "select" in g:
        select, W = so.update_w(V, int(g["k"]), str(g["metric"]), str(g["init"]))
        assert select == [int(s) for s in g["select"]]
        assert np.array_equal(W, g["W"])
    W = g["W"]
    H, ferr = so.update_h(V, W)
    assert np.abs(H - g["H"]).max() <= 1e-10
    assert abs(ferr - g["ferr"][0]) <= 1e-10 * max(1.0, g["ferr"][0])


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_h_is_a_kkt_point(name):
    g = load_golden(name)
    V = golden_v(g).astype(np.float64)
    _, _, S, F = so.products(V, g["W"])
    xmin, sum_dev, on, off = so.kkt_violation(S, F, g["H"])
    assert xmin >= 0.0
    assert sum_dev <= 1e-12
    assert on <= 1e-10          # the reduced gradient is equal on the support ...
    assert off <= 1e-10         # ... and not smaller off it


def test_origin_uses_the_last_column():
    g = load_golden("sivm_29x300_k6_origin")
    V = golden_v(g)
    assert int(g["select"][0]) == -1
    assert np.array_equal(g["W"][:, 0], V[:, -1].astype(np.float64))
