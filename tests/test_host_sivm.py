"""pymf_amd.SIVM without a GPU: the export, the constructor, the refusals, the -1 -> last column rule of the oracle."""
import os
import re

import numpy as np
import pytest

import pymf_amd
import sivm_oracle as so
from pymf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_sivm_get_select\(pmf_ctx\*\s*ctx,\s*int32_t\*\s*select\);", header)
    assert "PMF_ALGO_SIVM = 10" in header
    assert "pmf_sivm_get_select" in [s[0] for s in _lib.SYMBOLS]
    assert _lib.ALGO_SIVM == 10
    assert hasattr(_lib.Context, "get_select")


def test_constructor_defaults():
    data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    mdl = pymf_amd.SIVM(data)
    assert (mdl._num_bases, mdl._dist_measure, mdl._init) == (4, "l2", "fastmap")
    assert pymf_amd.SIVM._NITER == 1
    assert "SIVM" in pymf_amd.__all__
    mdl.init_w()
    mdl.init_h()
    assert np.array_equal(mdl.W, np.zeros((2, 4))) and np.array_equal(mdl.H, np.zeros((4, 3)))


@pytest.mark.parametrize("measure", ["kl", "abs_cosine", "weighted_abs_cosine"])
def test_unsupported_measures(measure):
    mdl = pymf_amd.SIVM(np.ones((3, 5)), num_bases=2, dist_measure=measure)
    for call in (mdl.factorize, mdl.update_w, mdl.update_h):
        with pytest.raises(NotImplementedError):
            call()


def test_refusals():
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(TypeError):
        pymf_amd.SIVM(sp.csr_matrix(np.ones((3, 5))), num_bases=2).factorize()
    mdl = pymf_amd.SIVM(np.ones((3, 5)), num_bases=2)
    mdl.stream_rows = 64
    with pytest.raises(ValueError):
        mdl.factorize()
    with pytest.raises(ValueError):
        pymf_amd.SIVM(np.ones((3, 100)), num_bases=65).factorize()
    with pytest.raises(ValueError):
        pymf_amd.SIVM(np.ones((3, 5)), num_bases=2, init="random").factorize()

    class World(object):
        size, rank = 2, 0

    mdl = pymf_amd.SIVM(np.ones((3, 5)), num_bases=2)
    mdl._world = lambda: World()
    with pytest.raises(NotImplementedError):
        mdl.factorize()


def test_minus_one_is_the_last_column():
    V = np.random.RandomState(3).random_sample((4, 9)) + 1.0
    select, W = so.update_w(V, 3, init="origin")
    assert select[0] == -1 and all(s >= 0 for s in select[1:])
    assert np.array_equal(W[:, 0], V[:, 8])
