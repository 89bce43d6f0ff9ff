"""pymf_amd.vq / pymf_amd.pdist without a GPU: the exports, the signatures, the refusals, which side becomes the data, and that
a model argument is served by the model's own context (a stand-in context, as in test_host_nmf_sparse.py)."""
import inspect
import os
import re
import warnings

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib
from pymf_amd import distance as mod
from pymf_amd.nmf import PrecisionWarning
from conftest import ROOT


class Ctx(object):
    """Records the calls of the two entries and answers with arrays of the right shape."""

    def __init__(self, m, n, log):
        self.m, self.n, self.log = m, n, log

    def set_v_dense(self, V):
        self.log.append(("set_v_dense", np.array(V)))

    def vq_columns(self, Q, metric=0, want_dist=True):
        self.log.append(("vq_columns", np.array(Q), metric))
        return np.arange(Q.shape[1], dtype=np.int32), None

    def vq_assign(self, Q, metric=0, want_idx=True, want_dist=False):
        self.log.append(("vq_assign", np.array(Q), metric, want_idx, want_dist))
        d = np.arange(Q.shape[1] * self.n, dtype=np.float64).reshape(Q.shape[1], self.n) if want_dist else None
        return (np.zeros(self.n, dtype=np.int32) if want_idx else None), d

    def close(self):
        self.log.append(("close",))


@pytest.fixture
def fake(monkeypatch):
    log = []
    monkeypatch.setattr(_lib, "Context", lambda algo, m, n, k: (log.append(("create", algo, m, n, k)), Ctx(m, n, log))[1])
    return log


def test_exports_and_signatures():
    assert pymf_amd.vq is mod.vq and pymf_amd.pdist is mod.pdist and pymf_amd.distance is mod
    for name in ("vq", "pdist", "distance", "dist"):
        assert name in pymf_amd.__all__
    assert mod.__all__ == ["vq", "pdist"]
    assert str(inspect.signature(mod.vq)) == "(A, B, metric='l2')"                 # dist.py:126
    assert str(inspect.signature(mod.pdist)) == "(A, B, metric='l2')"              # dist.py:107
    assert hasattr(pymf_amd.dist, "init_from_env")                                 # the rendezvous module stays what it is
    assert not hasattr(pymf_amd.dist, "vq")


def test_header_binding_and_integration_name_both_entries():
    header = open(os.path.join(ROOT, "include", "pymf_hip.h")).read()
    assert re.search(r"int\s+pmf_vq_columns\(pmf_ctx\*\s*ctx,\s*const float\*\s*Q,\s*int64_t\s+ldq,\s*int32_t\s+nq,\s*int32_t\s+metric,\s*"
                     r"int32_t\*\s*idx_out,\s*double\*\s*dist_out\);", header)
    assert re.search(r"int\s+pmf_vq_assign\(pmf_ctx\*\s*ctx,\s*const float\*\s*Q,\s*int64_t\s+ldq,\s*int32_t\s+nq,\s*int32_t\s+metric,\s*"
                     r"int32_t\*\s*idx_out,\s*double\*\s*dist_all\);", header)
    bound = [s[0] for s in _lib.SYMBOLS]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("pmf_vq_columns", "pmf_vq_assign"):
        assert name in bound and name in doc
    for name in ("vq_columns", "vq_assign"):
        assert hasattr(_lib.Context, name)
    assert mod.MAX_QUERIES == 128 and "1 <= nq <= 128" in open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_host_vq.h")).read()


def test_both_sides_over_128_columns(fake):
    A, B = np.ones((3, 129), dtype=np.float32), np.ones((3, 200), dtype=np.float32)
    for fn in (mod.vq, mod.pdist):
        with pytest.raises(ValueError, match="at most 128 columns"):
            fn(A, B)
    assert fake == []                                                              # refused before a context exists


def test_unknown_metric(fake):
    A, B = np.ones((3, 4), dtype=np.float32), np.ones((3, 9), dtype=np.float32)
    for fn in (mod.vq, mod.pdist):
        for metric in ("cosine", "kl", "L2", None, 0):
            with pytest.raises(ValueError, match="metric must be 'l2' or 'l1'"):
                fn(A, B, metric=metric)
    assert fake == []


def test_sparse_input(fake):
    import scipy.sparse as sp
    D, S = np.ones((3, 9), dtype=np.float32), sp.csr_matrix(np.ones((3, 4), dtype=np.float32))
    for fn in (mod.vq, mod.pdist):
        for a, b in ((S, D), (D, S), (S, S)):
            with pytest.raises(TypeError, match="scipy.sparse"):
                fn(a, b)
    with pytest.raises(ValueError, match="scipy.sparse"):                          # a model's sparse data: no dense image to measure
        mod.vq(pymf_amd.NMF(S, num_bases=2), D)
    assert fake == []


def test_shape_errors(fake):
    with pytest.raises(ValueError, match="dimensions differ"):
        mod.vq(np.ones((3, 4), dtype=np.float32), np.ones((5, 9), dtype=np.float32))
    with pytest.raises(ValueError, match="d x n"):
        mod.vq(np.ones(4, dtype=np.float32), np.ones((4, 2), dtype=np.float32))
    assert fake == []


def test_the_larger_side_is_uploaded_and_the_direction_follows(fake):
    rs = np.random.RandomState(0)
    small, large = rs.rand(3, 4).astype(np.float32), rs.rand(3, 300).astype(np.float32)
    out = mod.vq(small, large, metric="l1")                                        # samples B against centres A: assign
    assert [e[0] for e in fake] == ["create", "set_v_dense", "vq_assign", "close"]
    assert fake[0][2:] == (3, 300, 1) and np.array_equal(fake[1][1], large)
    assert np.array_equal(fake[2][1], small) and fake[2][2:] == (1, True, False)
    assert out.dtype == np.intp and out.shape == (300,)
    del fake[:]
    out = mod.vq(large, small)                                                     # bases B against data A: columns
    assert [e[0] for e in fake] == ["create", "set_v_dense", "vq_columns", "close"]
    assert np.array_equal(fake[1][1], large) and np.array_equal(fake[2][1], small) and fake[2][2] == 0
    assert out.dtype == np.intp and out.shape == (4,)
    del fake[:]
    d = mod.pdist(large, small)                                                    # nA x nB whichever side is the data
    assert d.shape == (300, 4) and d.flags.c_contiguous and d[7, 2] == 2 * 300 + 7
    d = mod.pdist(small, large)
    assert d.shape == (4, 300) and d[2, 7] == 2 * 300 + 7
    del fake[:]
    mod.vq(small, small.copy())                                                    # equal counts: A is looped over (dist.py:111)
    assert fake[2][0] == "vq_assign"


def test_float64_warns_once_per_call(fake):
    small, large = np.ones((3, 4)), np.ones((3, 300))
    for fn in (mod.vq, mod.pdist):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(small, large)
            fn(small.astype(np.float32), large)
        assert [x.category for x in w] == [PrecisionWarning, PrecisionWarning]
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(small.astype(np.float32), large.astype(np.float32))
        assert w == []


def test_a_model_argument_reuses_its_context(fake, monkeypatch):
    """vq(mdl, W): the model's `_sync_to_device()` context serves the call; no context is created, nothing is uploaded by
    vq itself, and the model's context is not closed."""
    rs = np.random.RandomState(1)
    data = rs.rand(5, 400).astype(np.float32)
    mdl = pymf_amd.SIVM(data, num_bases=3)
    mdl.W, mdl.H = np.zeros((5, 3)), np.zeros((3, 400))                            # a fitted model: data and factors are synchronised
    log = []
    own = Ctx(5, 400, log)
    monkeypatch.setattr(mdl, "_sync_to_device", lambda *a, **k: (log.append(("sync",)), own)[1])
    W = data[:, [7, 3, 9]]
    out = mod.vq(mdl, W)
    assert [e[0] for e in log] == ["sync", "vq_columns"] and fake == []
    assert np.array_equal(log[1][1], W) and list(out) == [0, 1, 2]
    del log[:]
    mod.vq(W, mdl, metric="l1")                                                    # the model as B: every sample to its centre
    assert [e[0] for e in log] == ["sync", "vq_assign"] and log[1][2:] == (1, True, False) and fake == []
    del log[:]
    assert mod.pdist(mdl, W).shape == (400, 3) and [e[0] for e in log] == ["sync", "vq_assign"]
    with pytest.raises(ValueError, match="at most 128 columns"):
        mod.vq(mdl, np.ones((5, 129), dtype=np.float32))
    mdl.stream_rows = 64
    with pytest.raises(ValueError, match="streamed"):
        mod.vq(mdl, W)


def test_a_model_without_factors_uploads_its_data_only(fake, monkeypatch):
    """A model whose W / H are not set yet: its own context with `_upload_data`, never `_sync_to_device` (which would raise the
    AttributeError of the missing W); a class that skips missing factors goes through `_sync_to_device` as it is."""
    data = np.random.RandomState(2).rand(5, 400).astype(np.float32)
    mdl = pymf_amd.NMF(data, num_bases=3)
    log = []
    own = Ctx(5, 400, log)
    monkeypatch.setattr(mdl, "_context", lambda: own)
    monkeypatch.setattr(mdl, "_upload_data", lambda ctx: log.append(("upload", ctx)))
    monkeypatch.setattr(mdl, "_sync_to_device", lambda *a, **k: pytest.fail("the factors are not needed"))
    mod.vq(mdl, data[:, :4])
    assert log[0] == ("upload", own) and log[1][0] == "vq_columns" and fake == []
    chn = pymf_amd.CHNMF(data, num_bases=3)                                        # _SKIP_MISSING_FACTORS
    del log[:]
    monkeypatch.setattr(chn, "_sync_to_device", lambda *a, **k: (log.append(("sync",)), own)[1])
    mod.vq(chn, data[:, :4])
    assert [e[0] for e in log] == ["sync", "vq_columns"]


def test_the_warning_points_at_the_caller_and_lists_count_as_float64(fake):
    small, large = [[1.0, 2.0], [3.0, 4.0]], np.ones((2, 300), dtype=np.float32)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        mod.vq(small, large)                                                       # (a list of floats is float64 data)
        mod.pdist(np.ones((2, 3), dtype=np.int32), large)                          # (integers convert exactly: no warning)
    assert [x.category for x in w] == [PrecisionWarning] and w[0].filename == __file__
