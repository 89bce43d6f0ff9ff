"""tests/aa_oracle.py against the goldens made by the real reference (tests/golden/gen_golden_aa.py): W, H and ferr everywhere,
beta only where num_samples <= data_dimension (elsewhere it is one of many minimisers).  The goldens pin aa.py's data flow, not
cvxopt's digits.  No GPU."""
import numpy as np
import pytest

import aa_cases as ac
import aa_oracle as ao
from conftest import load_golden

GOLDENS = ["aa_doc_2x3_k2", "aa_doc_userw", "aa_37x29_k5", "aa_29x300_k6"]


def start(g):
    """(V, W0, H0) of a golden: the seeded cases from aa_cases, the docstring cases from the reference's own draws."""
    if "case" in g:
        V, k, H0, W0 = ac.data(str(g["case"]))
        return V.astype(np.float64), W0, H0
    V = g["V"].astype(np.float64)
    k = int(g["k"])
    np.random.seed(int(g["seed"]))
    if bool(g["compute_w"]):                                   # nmf.py:173-177: init_w (beta, then W), then init_h
        b = np.random.random((k, V.shape[1]))
        W0 = np.random.random((V.shape[0], k))
    else:
        W0 = np.array([[1.0, 0.0], [0.0, 1.0]])
    H0 = np.random.random((k, V.shape[1]))
    H0 /= H0.sum(axis=0)
    return V, W0, H0


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_reproduces_golden(name):
    g = load_golden(name)
    assert bool(g["is_data_flow_pin"])
    V, W, H = start(g)
    ferr = []
    beta = None
    for _ in range(int(g["niter"])):
        if bool(g["compute_w"]):
            W, beta, _ = ao.update_w(V, H)
        H, f = ao.update_h(V, W)
        ferr.append(f)
        if len(ferr) > 2 and abs(ferr[-1] - ferr[-2]) / V.shape[1] < 1e-8:      # nmf.py:134-139,198-202
            ferr = ferr[:-1]
            break
    scale = max(1.0, np.abs(g["W"]).max())
    assert np.abs(W - g["W"]).max() <= 1e-8 * scale
    assert np.abs(H - g["H"]).max() <= 1e-7
    assert len(ferr) == len(g["ferr"])
    assert np.abs(np.array(ferr) - g["ferr"]).max() <= 1e-8 * max(1.0, g["ferr"].max())
    if beta is not None and V.shape[1] <= V.shape[0]:
        assert np.abs(beta - g["beta"]).max() <= 1e-8
    if beta is not None:
        assert np.abs(V.dot(g["beta"].T) - g["W"]).max() <= 1e-10 * scale           # aa.py:134
        assert g["beta"].min() >= -1e-12 and np.abs(g["beta"].sum(axis=1) - 1.0).max() <= 1e-10
