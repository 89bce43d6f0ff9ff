"""CUR / CMD on scipy.sparse data without a GPU: the export, the conversion that the classes hand to the device, the default
refusal, the classes that keep refusing whatever the flag says, and the limits."""
import os
import re

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib
from pymf_amd.cursl import CURSL
from pymf_amd.greedycur import GREEDYCUR
from pymf_amd.sivm_cur import SIVM_CUR

sp = pytest.importorskip("scipy.sparse")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder(object):
    """A context that takes set_v_csr and nothing else."""
    k = 128

    def __init__(self):
        self.calls = []

    def set_v_csr(self, indptr, indices, vals):
        self.calls.append((np.array(indptr), np.array(indices), np.array(vals)))

    def __getattr__(self, name):
        raise AssertionError("device call: %s" % name)


def data(fmt="csr", dtype=np.float32):
    return sp.random(20, 10, density=0.3, format=fmt, random_state=1, dtype=dtype)


def test_the_export_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_cur_ferr\(pmf_ctx\*\s*ctx,\s*double\*\s*out\);", header)
    assert "SNMF and NMF contexts only" not in header and "cur_csr" in header
    assert "pmf_cur_ferr" in [s[0] for s in _lib.SYMBOLS] and hasattr(_lib.Context, "cur_ferr")
    _lib.load()                                                # every declared symbol is in the library


def test_the_flag_is_a_class_attribute_and_off_by_default():
    for cls in (pymf_amd.CUR, pymf_amd.CMD):
        assert cls.accept_sparse is False
        with pytest.raises(TypeError):
            cls(data(), rrank=2).factorize()
        with pytest.raises(TypeError):
            cls(data(), rrank=2).computeUCR()
        with pytest.raises(TypeError):
            cls(data(), rrank=2).sample_probability()


@pytest.mark.parametrize("cls", [pymf_amd.CUR, pymf_amd.CMD])
@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_the_upload_hands_over_canonical_csr(cls, fmt):
    V = data(fmt, np.float64)
    mdl = cls(V, rrank=3)
    mdl.accept_sparse = True
    ctx = Recorder()
    mdl._ctx = ctx
    with pytest.warns(pymf_amd.nmf.PrecisionWarning):
        assert mdl._upload() is ctx
    assert len(ctx.calls) == 1                                 # set_v_csr, and never set_v_dense (the recorder has none)
    indptr, indices, vals = ctx.calls[0]
    ref = V.tocsr()
    ref.sum_duplicates()
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and vals.dtype == np.float32
    assert np.array_equal(indptr, ref.indptr) and np.array_equal(indices, ref.indices)
    assert np.array_equal(vals, ref.data.astype(np.float32))
    _lib.check_csr(20, 10, indptr, indices)
    assert all(np.all(np.diff(indices[indptr[r]:indptr[r + 1]]) > 0) for r in range(20))


def test_unsorted_indices_duplicates_and_stored_zeros():
    # row 0: columns 2, 0, 2 (unsorted, a duplicate); row 1: a stored zero
    indptr = np.array([0, 3, 4], dtype=np.int32)
    indices = np.array([2, 0, 2, 1], dtype=np.int32)
    vals = np.array([1.0, 5.0, 2.0, 0.0], dtype=np.float32)
    V = sp.csr_matrix((vals, indices, indptr), shape=(2, 3))
    mdl = pymf_amd.CUR(V, rrank=1)
    mdl.accept_sparse = True
    mdl._ctx = ctx = Recorder()
    mdl._upload()
    ip, ind, val = ctx.calls[0]
    assert ip.tolist() == [0, 2, 3] and ind.tolist() == [0, 2, 1] and val.tolist() == [5.0, 3.0, 0.0]   # the stored zero is kept
    assert V.nnz == 4 and V.data.tolist() == [1.0, 5.0, 2.0, 0.0]                                        # the caller's matrix keeps its entries


@pytest.mark.parametrize("cls", [CURSL, GREEDYCUR, SIVM_CUR])
def test_the_other_cur_classes_refuse_with_the_flag_set(monkeypatch, cls):
    def no_context(self, k=None):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(pymf_amd.CUR, "_context", no_context)
    mdl = cls(data(), rrank=2)
    mdl.accept_sparse = True
    with pytest.raises(TypeError):
        mdl.factorize()
    mdl._rid, mdl._rcnt, mdl._cid, mdl._ccnt = np.array([0]), np.ones(1), np.array([0]), np.ones(1)
    with pytest.raises(TypeError):
        mdl.computeUCR()


def test_svd_pca_and_pinv_refuse_with_the_flag_set(monkeypatch):
    monkeypatch.setattr(pymf_amd.SVD, "accept_sparse", True, raising=False)
    with pytest.raises(TypeError):
        pymf_amd.SVD(data()).factorize()
    with pytest.raises(TypeError):
        pymf_amd.svd.pinv(data())
    mdl = pymf_amd.PCA(data(), num_bases=2)
    mdl.accept_sparse = True
    with pytest.raises(TypeError):
        mdl.factorize(niter=1)


def test_a_multi_rank_world_and_a_rank_beyond_the_limit_are_refused(monkeypatch):
    big = sp.random(200, 300, density=0.1, format="csr", random_state=2, dtype=np.float32)
    for cls in (pymf_amd.CUR, pymf_amd.CMD):
        mdl = cls(big, rrank=129)
        mdl.accept_sparse = True
        with pytest.raises(ValueError):
            mdl.factorize()
        mdl = cls(big)                                         # rrank = 0: 200 rows, 300 columns
        mdl.accept_sparse = True
        with pytest.raises(ValueError):
            mdl.factorize()
    mdl = pymf_amd.CUR(big, rrank=2)
    mdl.accept_sparse = True
    mdl._rid, mdl._rcnt = np.arange(129), np.ones(129)
    mdl._cid, mdl._ccnt = np.arange(2), np.ones(2)
    with pytest.raises(ValueError):
        mdl.computeUCR()

    class World(object):
        size, rank, local_rank = 2, 0, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    for cls in (pymf_amd.CUR, pymf_amd.CMD):
        mdl = cls(big, rrank=2)
        mdl.accept_sparse = True
        with pytest.raises(NotImplementedError):
            mdl.factorize()


def test_frobenius_norm_wants_the_factors_of_the_last_call():
    mdl = pymf_amd.CUR(data(), rrank=2)
    mdl.accept_sparse = True
    with pytest.raises(AttributeError):
        mdl.frobenius_norm()                                   # before factorize(), as in the reference

    class Ferr(Recorder):
        def cur_ferr(self):
            return 1.5

    mdl._ctx = Ferr()
    mdl.U, mdl.S, mdl.V = np.ones((20, 2)), np.ones((2, 2)), np.ones((2, 10))
    mdl._on_device = (mdl.U, mdl.S, mdl.V)
    assert mdl.frobenius_norm() == 1.5
    for name in "USV":
        keep = getattr(mdl, name)
        setattr(mdl, name, keep.copy())
        with pytest.raises(NotImplementedError, match=name + " was rebound"):
            mdl.frobenius_norm()
        setattr(mdl, name, keep)
