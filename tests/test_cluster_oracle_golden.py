"""tests/cluster_oracle.py against the goldens written by the real reference (tests/golden/gen_golden_cluster.py).  No GPU."""
import random

import numpy as np
import pytest

import cluster_oracle as co
from cluster_cases import CMEANS_GOLDENS, KMEANS_GOLDENS, load_case, onehot


@pytest.mark.parametrize("name", KMEANS_GOLDENS)
def test_kmeans_oracle_matches_the_reference(name):
    g = load_case(name)
    V, k = g["V"].astype(np.float64), int(g["k"])
    random.seed(int(g["random_seed"]))
    sel = random.sample(range(V.shape[1]), k)                     # kmeans.py:69
    ce = bool(g["compute_err"])
    W, H, assigned, ferr, gap = co.kmeans(V, k, sel=sel, niter=int(g["niter"]), compute_err=ce)
    assert np.array_equal(assigned, g["assigned"])
    np.testing.assert_allclose(W, g["W"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(H, onehot(g["assigned"], k))
    if ce:
        assert len(ferr) == len(g["ferr"])
        np.testing.assert_allclose(ferr, g["ferr"], rtol=1e-12, atol=1e-12)
    assert float(g["min_gap"]) >= 1e-4
    np.testing.assert_allclose(gap, float(g["min_gap"]), rtol=1e-9)


@pytest.mark.parametrize("name", CMEANS_GOLDENS)
def test_cmeans_oracle_matches_the_reference(name):
    g = load_case(name)
    V, k = g["V"].astype(np.float64), int(g["k"])
    m, n = V.shape
    np.random.seed(int(g["np_seed"]))
    if "W_user" in g:
        W0 = g["W_user"]
    else:
        W0 = np.random.random((m, k))                             # nmf.py:116-117
    H0 = np.random.random((k, n))                                 # nmf.py:119-120
    W, H, ferr = co.cmeans(V, W0, H0, niter=int(g["niter"]), compute_w=bool(g["compute_w"]))
    assert len(ferr) == len(g["ferr"])
    np.testing.assert_allclose(W, g["W"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(H, g["H"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ferr, g["ferr"], rtol=1e-12, atol=1e-12)
