"""pymf_amd.AA without a GPU: the export, the refusals, the draws of init_w / init_h against the reference's stream."""
import os
import re

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_aa_get_beta\(pmf_ctx\*\s*ctx,\s*double\*\s*beta\);", header)
    assert "PMF_ALGO_AA = 11" in header
    assert "pmf_aa_get_beta" in [s[0] for s in _lib.SYMBOLS]
    assert _lib.ALGO_AA == 11
    assert hasattr(_lib.Context, "get_beta")
    assert "AA" in pymf_amd.__all__
    assert issubclass(pymf_amd.AA, pymf_amd.NMF) and not issubclass(pymf_amd.SIVM, pymf_amd.AA)


def test_constructor_defaults():
    mdl = pymf_amd.AA(np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]]))
    assert mdl._num_bases == 4 and (mdl._data_dimension, mdl._num_samples) == (2, 3)


def test_draws_follow_the_reference_stream():
    """aa.py:83-91: init_w draws beta (k x n, normalised per column) and then W (m x k); init_h draws H and normalises it."""
    m, n, k = 5, 7, 3
    np.random.seed(42)
    b = np.random.random((k, n))
    b /= b.sum(axis=0)
    W = np.random.random((m, k))
    H = np.random.random((k, n))
    H /= H.sum(axis=0)
    after = np.random.random()
    mdl = pymf_amd.AA(np.ones((m, n)), num_bases=k)
    np.random.seed(42)
    mdl.init_w()
    mdl.init_h()
    assert np.array_equal(mdl.beta, b) and np.array_equal(mdl.W, W) and np.array_equal(mdl.H, H)
    assert np.random.random() == after
    assert mdl.W.shape == (m, k) and mdl.beta.shape == (k, n)
    assert np.allclose(mdl.H.sum(axis=0), 1.0) and np.allclose(mdl.beta.sum(axis=0), 1.0)


def test_refusals():
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(TypeError):
        pymf_amd.AA(sp.csr_matrix(np.ones((3, 5))), num_bases=2).factorize()
    mdl = pymf_amd.AA(np.ones((3, 5)), num_bases=2)
    mdl.stream_rows = 64
    for call in (mdl.factorize, mdl.update_w, mdl.update_h, mdl.frobenius_norm):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        pymf_amd.AA(np.ones((3, 100)), num_bases=65).factorize()

    class World(object):
        size, rank = 2, 0

    mdl = pymf_amd.AA(np.ones((3, 5)), num_bases=2)
    mdl._world = lambda: World()
    with pytest.raises(NotImplementedError):
        mdl.factorize()


def test_corral_bound_is_named():
    with pytest.raises(ValueError, match=r"min\(data_dimension \+ 1, num_samples\) > 128"):
        pymf_amd.AA(np.ones((128, 200)), num_bases=2).factorize()
    pymf_amd.AA(np.ones((127, 200)), num_bases=2)._check_supported()          # 128 columns at most: allowed
    pymf_amd.AA(np.ones((5000, 128)), num_bases=2)._check_supported()
