"""pymf_amd.CUR / CMD / pinv without a GPU: exports, constructor attributes, refusals, CMD's merge of repeated indices."""
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
    assert re.search(r"int\s+pmf_cur_sqnorms\(pmf_ctx\*\s*ctx,\s*double\*\s*row_sq,\s*double\*\s*col_sq\);", header)
    assert re.search(r"int\s+pmf_cur_compute\(pmf_ctx\*\s*ctx,\s*const int32_t\*\s*rid,\s*const int32_t\*\s*rcnt,\s*int32_t nr,\s*"
                     r"const int32_t\*\s*cid,\s*const int32_t\*\s*ccnt,\s*int32_t nc\);", header)
    assert re.search(r"int\s+pmf_cur_get\(pmf_ctx\*\s*ctx,\s*double\*\s*C,\s*double\*\s*U,\s*double\*\s*R\);", header)
    assert "PMF_ALGO_CUR = 14" in header
    bound = [s[0] for s in _lib.SYMBOLS]
    assert "pmf_cur_sqnorms" in bound and "pmf_cur_compute" in bound and "pmf_cur_get" in bound
    assert _lib.ALGO_CUR == 14
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "pmf_cur_sqnorms" in doc and "pmf_cur_compute" in doc and "pmf_cur_get" in doc
    assert "CUR" in pymf_amd.__all__ and "CMD" in pymf_amd.__all__ and "pinv" in pymf_amd.__all__
    assert callable(pymf_amd.pinv) and pymf_amd.pinv is pymf_amd.svd.pinv
    assert issubclass(pymf_amd.CMD, pymf_amd.CUR) and issubclass(pymf_amd.CUR, pymf_amd.SVD)


def test_context_limits():
    def code(*args):
        try:
            _lib.Context(*args).close()
        except _lib.PmfError as e:
            return e.code
        return _lib.PMF_OK
    assert code(_lib.ALGO_CUR, 300, 400, 129) == _lib.PMF_EINVAL             # more than 128 sampled rows / columns
    assert code(_lib.ALGO_CUR, 300, 400, 0) == _lib.PMF_EINVAL
    assert code(13, 30, 40, 5) == _lib.PMF_EINVAL                            # 13 stays unassigned
    assert code(_lib.ALGO_CUR, 30, 40, 5, 0, 0, 2, b"x" * _lib.NCCL_ID_BYTES) == _lib.PMF_EINVAL   # one rank only
    ok = code(_lib.ALGO_CUR, 300, 400, 128)
    assert ok == (_lib.PMF_OK if _lib.device_count() > 0 else _lib.PMF_EHIP)


@pytest.mark.parametrize("cls", [pymf_amd.CUR, pymf_amd.CMD])
def test_constructor_attributes(cls):
    mdl = cls(DOC, rrank=1, crank=2)
    # cur.py:60 hands crank=rrank to SVD.__init__: the crank argument is ignored
    assert (mdl._rows, mdl._cols, mdl._rrank, mdl._crank, mdl._k) == (2, 3, 1, 1, -1)
    assert mdl._crank == mdl._rrank
    assert mdl.data is DOC and cls._EPS == 1e-8
    assert mdl._rset == range(2) and mdl._cset == range(3)
    mdl = cls(DOC)                                             # rrank = 0: all rows, all columns
    assert (mdl._rrank, mdl._crank) == (2, 3)
    mdl = cls(DOC, k=2, crank=2)
    assert (mdl._rrank, mdl._crank, mdl._k) == (2, 3, 2)
    with pytest.raises(AttributeError):
        mdl.frobenius_norm()                                   # no U yet, as in the reference
    for name in ("sample", "sample_probability", "computeUCR", "factorize"):
        assert callable(getattr(mdl, name))


def test_refusals(monkeypatch):
    sp = pytest.importorskip("scipy.sparse")
    for cls in (pymf_amd.CUR, pymf_amd.CMD):
        with pytest.raises(TypeError):
            cls(sp.csr_matrix(np.ones((3, 5))), rrank=2).factorize()
        with pytest.raises(ValueError):
            cls(np.ones((200, 300), dtype=np.float32), rrank=129).factorize()
        with pytest.raises(ValueError):
            cls(np.ones((200, 300), dtype=np.float32)).factorize()         # rrank = 0: 200 rows, 300 columns
    mdl = pymf_amd.CUR(np.ones((300, 5), dtype=np.float32), rrank=2)
    mdl._rid, mdl._rcnt = np.arange(129), np.ones(129)
    mdl._cid, mdl._ccnt = np.arange(2), np.ones(2)
    with pytest.raises(ValueError):
        mdl.computeUCR()
    mdl._rid, mdl._rcnt = np.array([0, 300]), np.ones(2)
    with pytest.raises(IndexError):
        mdl.computeUCR()
    mdl._rid, mdl._rcnt = np.array([0, -301]), np.ones(2)
    with pytest.raises(IndexError):
        mdl.computeUCR()
    mdl._rid, mdl._rcnt = np.array([0, 1]), np.array([1.0, 0.0])
    with pytest.raises(ValueError):
        mdl.computeUCR()

    class World(object):
        size, rank, local_rank = 2, 0, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    for cls in (pymf_amd.CUR, pymf_amd.CMD):
        with pytest.raises(NotImplementedError):
            cls(np.ones((3, 5), dtype=np.float32), rrank=2).factorize()
    with pytest.raises(NotImplementedError):
        mdl.computeUCR()


def test_cmdinit_on_a_hand_made_index_list():
    mdl = pymf_amd.CMD(np.ones((12, 9)), rrank=6)
    mdl._rid = np.int32([2, 2, 5, 9, 9, 9])
    mdl._cid = np.int32([0, 3, 3, 3, 3, 8])
    mdl._cmdinit()
    assert mdl._rid.tolist() == [2, 5, 9] and mdl._rid.dtype == np.int32
    assert mdl._cid.tolist() == [0, 3, 8] and mdl._cid.dtype == np.int32
    assert mdl._rcnt.tolist() == [2.0, 1.0, 3.0] and mdl._ccnt.tolist() == [1.0, 4.0, 1.0]


def test_sample_follows_the_reference():
    mdl = pymf_amd.CUR(DOC, rrank=1)
    probs = np.array([[0.2], [0.5], [0.3]])
    np.random.seed(4)
    draws = [np.random.rand() for _ in range(6)]
    np.random.seed(4)
    got = mdl.sample(6, probs)
    cum = np.cumsum(probs.flatten())
    assert got.dtype == np.int32 and got.tolist() == sorted(int(np.where(cum >= v)[0][0]) for v in draws)
    np.random.seed(0)
    with pytest.raises(IndexError):
        mdl.sample(3, np.array([0.1, 0.1]))                    # every draw here exceeds the last cumulative value


def test_pinv_has_svds_limits():
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(TypeError):
        pymf_amd.pinv(sp.csr_matrix(np.ones((3, 5))))
    with pytest.raises(ValueError):
        pymf_amd.pinv(np.zeros((2433, 2433), dtype=np.float32))
