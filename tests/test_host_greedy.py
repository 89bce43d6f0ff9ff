"""pymf_amd.GREEDY / GREEDYCUR without a GPU: exports, constructor attributes, refusals."""
import os
import re

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])


def test_exports_are_declared_bound_and_documented():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_greedy_select\(pmf_ctx\*\s*ctx,\s*int32_t transposed,\s*int32_t nsel,\s*int32_t\*\s*select\);", header)
    assert "PMF_ALGO_GREEDY = 15" in header
    assert "pmf_greedy_select" in [s[0] for s in _lib.SYMBOLS]
    assert _lib.ALGO_GREEDY == 15
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "pmf_greedy_select" in doc and "GREEDYCUR" in doc
    assert "GREEDY" in pymf_amd.__all__ and "GREEDYCUR" in pymf_amd.__all__
    assert issubclass(pymf_amd.GREEDY, pymf_amd.NMF) and issubclass(pymf_amd.GREEDYCUR, pymf_amd.CUR)


def test_context_limits():
    def code(*args):
        try:
            _lib.Context(*args).close()
        except _lib.PmfError as e:
            return e.code
        return _lib.PMF_OK
    assert code(_lib.ALGO_GREEDY, 30, 400, 65) == _lib.PMF_EINVAL             # more than 64 bases
    assert code(_lib.ALGO_GREEDY, 2433, 2433, 4) == _lib.PMF_EINVAL           # the short side
    assert code(16, 30, 40, 5) == _lib.PMF_EINVAL                            # 16 is not assigned
    assert code(_lib.ALGO_GREEDY, 30, 40, 5, 0, 0, 2, b"x" * _lib.NCCL_ID_BYTES) == _lib.PMF_EINVAL   # one rank only
    ok = code(_lib.ALGO_GREEDY, 2432, 100000, 64)
    assert ok == (_lib.PMF_OK if _lib.device_count() > 0 else _lib.PMF_EHIP)


def test_constructor_attributes():
    mdl = pymf_amd.GREEDY(DOC, num_bases=2)
    assert (mdl._data_dimension, mdl._num_samples, mdl._num_bases, mdl._k) == (2, 3, 2, 2)
    assert pymf_amd.GREEDY(DOC, k=7, num_bases=2)._k == 7
    assert mdl.data is DOC and not hasattr(mdl, "select")
    assert pymf_amd.GREEDY.init_w is pymf_amd.NMF.init_w and pymf_amd.GREEDY.init_h is pymf_amd.NMF.init_h
    assert mdl.frobenius_norm() == -123456                     # no W, H yet (nmf.py:100-114)
    cur = pymf_amd.GREEDYCUR(DOC, rrank=1, crank=2)
    assert (cur._rows, cur._cols, cur._rrank, cur._crank, cur._k) == (2, 3, 1, 1, -1)   # crank follows rrank (cur.py:60)
    for name in ("sample", "computeUCR", "factorize"):
        assert callable(getattr(cur, name))


def test_refusals(monkeypatch):
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(TypeError):
        pymf_amd.GREEDY(sp.csr_matrix(np.ones((3, 5))), num_bases=2).factorize()
    with pytest.raises(ValueError):
        pymf_amd.GREEDY(np.ones((8, 100), dtype=np.float32), num_bases=65).factorize()
    with pytest.raises(ValueError):
        pymf_amd.GREEDY(np.ones((2433, 2433), dtype=np.float32), num_bases=2).update_w()
    mdl = pymf_amd.GREEDY(np.ones((8, 100), dtype=np.float32), num_bases=2)
    mdl.stream_rows = 64
    with pytest.raises(ValueError):
        mdl.factorize()
    with pytest.raises(AttributeError):
        pymf_amd.GREEDY(np.ones((8, 100), dtype=np.float32), num_bases=2).update_h()      # no W
    with pytest.raises(TypeError):
        pymf_amd.GREEDYCUR(sp.csr_matrix(np.ones((3, 5))), rrank=2).factorize()
    with pytest.raises(ValueError):
        pymf_amd.GREEDYCUR(np.ones((80, 100), dtype=np.float32), rrank=65).factorize()
    with pytest.raises(ValueError):
        pymf_amd.GREEDYCUR(np.ones((80, 100), dtype=np.float32)).factorize()            # rrank = 0: 80 rows, 100 columns
    with pytest.raises(ValueError):
        pymf_amd.GREEDYCUR(np.ones((2433, 2433), dtype=np.float32), rrank=2).factorize()

    class World(object):
        size, rank, local_rank = 2, 0, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    with pytest.raises(NotImplementedError):
        pymf_amd.GREEDY(np.ones((3, 5), dtype=np.float32), num_bases=2).factorize()
    with pytest.raises(NotImplementedError):
        pymf_amd.GREEDYCUR(np.ones((3, 5), dtype=np.float32), rrank=2).factorize()
