"""SIVM on scipy.sparse data without a GPU: the exports, the host-only check of the CSC arrays (pmf_check_csc), the
conversion that the classes hand to the device, compute_err and frobenius_norm, and the classes that keep refusing."""
import os
import re

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

sp = pytest.importorskip("scipy.sparse")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder(object):
    """A context that takes set_v_csc and nothing else."""

    def __init__(self):
        self.calls = []

    def set_v_csc(self, indptr, indices, vals):
        self.calls.append((np.array(indptr), np.array(indices), np.array(vals)))

    def __getattr__(self, name):
        raise AssertionError("device call: %s" % name)


def data(fmt="csc", dtype=np.float32):
    return sp.random(20, 10, density=0.3, format=fmt, random_state=1, dtype=dtype)


def test_exports_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_set_v_csc_f32\(pmf_ctx\*\s*ctx,\s*const int64_t\*\s*indptr,\s*const int32_t\*\s*indices,\s*const float\*\s*vals,\s*int64_t nnz\);", header)
    assert re.search(r"int\s+pmf_check_csc\(", header) and "sivm_csc_team" in header
    names = [s[0] for s in _lib.SYMBOLS]
    assert "pmf_set_v_csc_f32" in names and "pmf_check_csc" in names
    assert hasattr(_lib.Context, "set_v_csc")
    _lib.load()                                                # every declared symbol is in the library


def test_the_host_check_of_the_arrays():
    V = data()
    _lib.check_csc(20, 10, V.indptr, V.indices)                # canonical arrays pass
    _lib.check_csc(3, 2, [0, 0, 0], [])                        # an empty matrix too

    def refused(indptr, indices, why, m=20, n=10):
        with pytest.raises(_lib.PmfError, match=why) as e:
            _lib.check_csc(m, n, indptr, indices)
        assert e.value.code == _lib.PMF_EINVAL

    ip = V.indptr.copy()
    ip[3], ip[4] = ip[4] + 1, ip[3]
    refused(ip, V.indices, "indptr must not decrease")
    ip = V.indptr.copy()
    ip[-1] -= 1
    refused(ip, V.indices, "indptr\\[n\\] must be nnz")
    ip = V.indptr.copy()
    ip[0] = 1
    refused(ip, V.indices, "indptr\\[0\\] must be 0")
    bad = V.indices.copy()
    bad[5] = 20
    refused(V.indptr, bad, "row index out of range")
    bad = V.indices.copy()
    bad[5] = -1
    refused(V.indptr, bad, "row index out of range")
    refused([0, 2], [1, 0], "must ascend", m=3, n=1)           # unsorted
    refused([0, 2], [1, 1], "must ascend", m=3, n=1)           # a duplicate


@pytest.mark.parametrize("fmt", ["csc", "csr", "coo"])
def test_the_upload_hands_over_canonical_csc(fmt):
    cls = pymf_amd.SIVM
    V = data(fmt, np.float64)
    mdl = cls(V, num_bases=2)
    ctx = Recorder()
    with pytest.warns(pymf_amd.nmf.PrecisionWarning):
        mdl._upload_data(ctx)
    mdl._upload_data(ctx)                                      # unchanged: the digest of the three arrays spares the upload
    assert len(ctx.calls) == 1
    indptr, indices, vals = ctx.calls[0]
    ref = V.tocsc()
    ref.sum_duplicates()
    assert np.array_equal(indptr, ref.indptr) and np.array_equal(indices, ref.indices) and np.array_equal(vals, ref.data)
    _lib.check_csc(20, 10, indptr, indices)
    if fmt != "coo":
        V.data[0] += 1.0                                       # an in-place edit is noticed
        mdl._upload_data(ctx)
        assert len(ctx.calls) == 2 and not np.array_equal(ctx.calls[1][2], vals)


def test_unsorted_indices_duplicates_and_stored_zeros():
    # column 0: rows 2, 0, 2 (unsorted, a duplicate); column 1: a stored zero
    indptr = np.array([0, 3, 4], dtype=np.int32)
    indices = np.array([2, 0, 2, 1], dtype=np.int32)
    vals = np.array([1.0, 5.0, 2.0, 0.0], dtype=np.float32)
    V = sp.csc_matrix((vals, indices, indptr), shape=(3, 2))
    mdl = pymf_amd.SIVM(V, num_bases=1)
    ctx = Recorder()
    mdl._upload_data(ctx)
    ip, ind, val = ctx.calls[0]
    assert ip.tolist() == [0, 2, 3] and ind.tolist() == [0, 2, 1] and val.tolist() == [5.0, 3.0, 0.0]   # the stored zero is kept
    assert V.nnz == 4 and V.data.tolist() == [1.0, 5.0, 2.0, 0.0]                                        # the caller's matrix keeps its entries
    _lib.check_csc(3, 2, ip, ind)


def test_compute_err_is_refused_before_any_device_call_and_the_norm_is_the_sentinel(monkeypatch):
    cls = pymf_amd.SIVM
    def no_context(self):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(pymf_amd.NMF, "_context", no_context)
    mdl = cls(data(), num_bases=2)
    with pytest.raises(TypeError, match="compute_err=False"):
        mdl.factorize()                                        # compute_err=True is the default
    assert mdl.frobenius_norm() == -123456
    mdl.W, mdl.H = np.ones((20, 2)), np.ones((2, 10))
    assert mdl.frobenius_norm() == -123456


@pytest.mark.parametrize("name", ["LAESA", "GMAP", "SIVM_SGREEDY", "SIVM_GSAT", "SIVM_CUR"])
def test_the_other_classes_still_refuse_sparse_data(monkeypatch, name):
    def no_context(self):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(pymf_amd.NMF, "_context", no_context)
    cls = getattr(pymf_amd, name, None) or getattr(__import__("pymf_amd.%s" % name.lower(), fromlist=[name]), name)
    mdl = cls(data(), **({"rrank": 2, "crank": 2} if name == "SIVM_CUR" else {"num_bases": 2}))
    with pytest.raises(TypeError):
        mdl.factorize(**({} if name == "SIVM_CUR" else {"compute_err": False}))
    assert pymf_amd.SIVM._TAKES_SPARSE and not pymf_amd.LAESA._TAKES_SPARSE
