"""pymf_amd.SIVM_CUR without a GPU: export, signature, constructor attributes, refusals before any device call."""
import inspect
import os
import re

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])


def test_exports_are_declared_bound_and_documented():
    assert "SIVM_CUR" in pymf_amd.__all__ and issubclass(pymf_amd.SIVM_CUR, pymf_amd.CUR)
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_sivm_select\(pmf_ctx\*\s*ctx,\s*int32_t transposed,\s*int32_t nsel,\s*int32_t metric,\s*int32_t init,\s*"
                     r"int32_t path,\s*int32_t\*\s*select\);", header)
    assert "pmf_sivm_select" in [s[0] for s in _lib.SYMBOLS]
    sig = inspect.signature(_lib.Context.sivm_select)
    assert list(sig.parameters) == ["self", "nsel", "transposed", "metric", "init", "path"] and sig.parameters["path"].default == 0
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "pmf_sivm_select" in doc and "SIVM_CUR" in doc


def test_signature_and_defaults():
    sig = inspect.signature(pymf_amd.SIVM_CUR.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [
        ("k", -1), ("rrank", 0), ("crank", 0), ("dist_measure", "l2"), ("init", "origin")]   # sivm_cur.py:60
    mdl = pymf_amd.SIVM_CUR(DOC, rrank=1, crank=2)
    assert (mdl._rows, mdl._cols, mdl._rrank, mdl._crank, mdl._k) == (2, 3, 1, 1, -1)          # crank follows rrank (cur.py:60)
    assert mdl._dist_measure == "l2" and mdl.init == "origin" and mdl.data is DOC
    all_ = pymf_amd.SIVM_CUR(np.ones((5, 7)))
    assert (all_._rrank, all_._crank) == (5, 7)                                             # rrank = 0: all rows and columns
    for name in ("sample", "computeUCR", "factorize"):
        assert callable(getattr(mdl, name))


def test_refusals_come_before_any_device_call(monkeypatch):
    sp = pytest.importorskip("scipy.sparse")

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "Context", no_device)
    small = np.ones((8, 100), dtype=np.float32)
    with pytest.raises(TypeError):
        pymf_amd.SIVM_CUR(sp.csr_matrix(np.ones((3, 5))), rrank=2).factorize()
    with pytest.raises(ValueError):
        pymf_amd.SIVM_CUR(np.ones((80, 100), dtype=np.float32), rrank=65).factorize()
    with pytest.raises(ValueError):
        pymf_amd.SIVM_CUR(np.ones((80, 100), dtype=np.float32)).factorize()                # rrank = 0: 80 rows, 100 columns
    with pytest.raises(ValueError):
        pymf_amd.SIVM_CUR(np.broadcast_to(np.float32(1.0), (16385, 16385)), rrank=2).factorize()
    with pytest.raises(ValueError):
        pymf_amd.SIVM_CUR(small, rrank=2).sample(small, 65)
    for measure in ("kl", "abs_cosine", "weighted_abs_cosine"):
        with pytest.raises(NotImplementedError):
            pymf_amd.SIVM_CUR(small, rrank=2, dist_measure=measure).factorize()
        with pytest.raises(NotImplementedError):
            pymf_amd.SIVM_CUR(small, rrank=2, dist_measure=measure).sample(small, 2)
    with pytest.raises(ValueError):
        pymf_amd.SIVM_CUR(small, rrank=2, dist_measure="l3").factorize()
    with pytest.raises(ValueError):
        pymf_amd.SIVM_CUR(small, rrank=2, init="random").factorize()

    class World(object):
        size, rank, local_rank = 2, 0, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    with pytest.raises(NotImplementedError):
        pymf_amd.SIVM_CUR(small, rrank=2).factorize()


def test_sample_recognises_the_transposed_view(monkeypatch):
    """The data and its transposed view (same address, reversed strides) run on the resident copy; anything else -- a copy of
    the transposed data, another matrix of that shape -- goes through a SIVM object of its own."""
    calls = []

    class Ctx(object):
        k = 8

        def set_v_dense(self, arr):
            calls.append(("upload", arr.shape))

        def sivm_select(self, nsel, transposed=False, metric=0, init=0, path=0):
            calls.append(("select", nsel, transposed, metric, init, path))
            return np.arange(nsel, dtype=np.int32) - 1

        def close(self):
            pass

    class FakeSIVM(object):
        def __init__(self, data, num_bases=4, dist_measure="l2", init="fastmap"):
            calls.append(("SIVM", data.shape, num_bases, dist_measure, init))
            self.select = [7] * num_bases

        def factorize(self, **kw):
            calls.append(("factorize", kw.get("compute_h"), kw.get("compute_err")))

    import pymf_amd.sivm_cur as m
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: Ctx())
    monkeypatch.setattr(m, "SIVM", FakeSIVM)
    d = np.arange(12.0, dtype=np.float32).reshape(3, 4)
    mdl = pymf_amd.SIVM_CUR(d, rrank=2, dist_measure="cosine", init="fastmap")
    out = mdl.sample(d.transpose(), 2)
    assert out == [-1, 0] and all(type(s) is int for s in out)
    assert calls == [("upload", (3, 4)), ("select", 2, True, 2, 0, 0)]
    assert mdl.sample(d, 2) == [-1, 0] and calls[2:] == [("select", 2, False, 2, 0, 0)]      # one upload serves both
    del calls[:]
    assert mdl.sample(d.T.copy(), 2) == [7, 7]
    assert calls == [("SIVM", (4, 3), 2, "cosine", "fastmap"), ("factorize", False, False)]
    del calls[:]
    assert mdl.sample(np.ones((4, 3), dtype=np.float32), 2) == [7, 7] and calls[0][0] == "SIVM"


def test_factorize_has_no_cpu_fallback():
    mdl = pymf_amd.SIVM_CUR(DOC.astype(np.float32), rrank=1)
    if _lib.device_count() > 0:
        mdl.factorize()
        assert mdl._rid == [-1] and mdl._cid == [-1]
    else:
        with pytest.raises(_lib.PmfError):
            mdl.factorize()
