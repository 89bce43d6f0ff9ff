"""pymf_amd.SUB without a GPU: the export, the signature, the strategy dispatch, every refusal before any device call, the
'rand' and 'cur' draws, where each model's device V comes from (stand-in contexts, as in test_host_nmf_sparse.py) and the two
C-ABI entries in header, binding and library."""
import inspect
import os
import random
import re

import numpy as np
import pytest

import pymf_amd
import sub_cases as sc
from pymf_amd import _lib
from pymf_amd import dist as _dist
from pymf_amd import sub as mod
from conftest import ROOT


class Ctx(object):
    """Records where V comes from; answers cur_sqnorms with the norms it was given.  Anything else is a device call the test did
    not expect."""
    norms = None

    def __init__(self, algo, m, n, k, log):
        self.algo, self.m, self.n, self.k, self.log = algo, m, n, k, log

    def set_v_dense(self, V):
        self.log.append(("set_v_dense", self, np.array(V)))

    def set_v_gather(self, src, idx=None):
        self.log.append(("set_v_gather", self, src, None if idx is None else np.array(idx)))

    def cur_sqnorms(self):
        self.log.append(("cur_sqnorms", self))
        return np.zeros(self.m), np.array(Ctx.norms, dtype=np.float64)

    def __getattr__(self, name):
        raise AssertionError("device call: %s" % name)


@pytest.fixture
def fake(monkeypatch):
    log = []
    monkeypatch.setattr(_dist, "make_context", lambda algo, m, n, k: Ctx(algo, m, n, k, log))
    return log


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_dist, "make_context", refuse)
    monkeypatch.setattr(_lib, "Context", refuse)


def data(rows=6, n=40):
    return sc.sub_data(rows, n)


def test_export_signature_and_attributes():
    assert pymf_amd.SUB is mod.SUB and "SUB" in pymf_amd.__all__ and mod.__all__ == ["SUB"]
    assert str(inspect.signature(mod.SUB.__init__)) == ("(self, data, mfmethod, nsub=20, show_progress=True, mapW=False, base_sel=2, "
                                                        "num_bases=3, niterH=1, compute_h=True, compute_w=True, sstrategy='rand')")   # sub.py:49-50
    assert str(inspect.signature(mod.SUB.factorize)) == "(self)"                  # sub.py:206
    V = data()
    mdl = pymf_amd.SUB(V, pymf_amd.NMF)
    assert (mdl._niterH, mdl._nsub, mdl._mfmethod, mdl._mapW, mdl._sstrategy, mdl._base_sel) == (1, 20, pymf_amd.NMF, False, 'rand', 2)
    assert mdl.data is V and mdl._num_bases == 3 and (mdl._data_dimension, mdl._num_samples) == V.shape
    assert not hasattr(mdl, "mdl") and mdl.frobenius_norm() == -123456


def test_subfunc_dispatch():
    V = data()
    for name, attr in (("cur", "curselect"), ("kmeans", "kmeansselect"), ("hull", "hullselect"), ("laesa", "laesaselect"),
                       ("sivm", "sivmselect"), ("rand", "randselect"), ("no such strategy", "randselect")):
        mdl = pymf_amd.SUB(V, pymf_amd.NMF, sstrategy=name)                     # (the constructor accepts every name)
        assert mdl._subfunc == getattr(mdl, attr), name
        assert mdl._sstrategy == name


def test_mfmethod_must_be_a_model_class(no_device):
    for bad in (dict, pymf_amd.NMF(data(), num_bases=2), "NMF", None, pymf_amd.vq, pymf_amd.SUB):
        with pytest.raises(TypeError, match="mfmethod must be a pymf_amd model class"):
            pymf_amd.SUB(data(), bad)


def test_refusals_come_before_any_device_call(no_device, monkeypatch):
    V = data()
    for strategy in ("rand", "kmeans", "sivm", "laesa", "cur"):
        mdl = pymf_amd.SUB(V, pymf_amd.NMF, nsub=4, sstrategy=strategy)
        mdl.stream_rows = 64
        with pytest.raises(ValueError, match="streamed data"):
            mdl.factorize()
    monkeypatch.setenv("PYMF_STREAM_ROWS", "64")
    with pytest.raises(ValueError, match="streamed data"):
        pymf_amd.SUB(V, pymf_amd.NMF, nsub=4).factorize()
    monkeypatch.delenv("PYMF_STREAM_ROWS")
    monkeypatch.setattr(_dist, "_WORLD", _dist.World(0, 2))
    with pytest.raises(NotImplementedError, match="one rank only"):
        pymf_amd.SUB(V, pymf_amd.NMF, nsub=4).factorize()
    monkeypatch.setattr(_dist, "_WORLD", _dist.World())
    for nsub in (0, -1, V.shape[1] + 1):
        with pytest.raises(ValueError):
            pymf_amd.SUB(V, pymf_amd.NMF, nsub=nsub).factorize()
    with pytest.raises(ValueError, match=r"'kmeans' takes nsub <= 128 \(Kmeans"):
        pymf_amd.SUB(sc.sub_data(4, 200), pymf_amd.NMF, nsub=129, sstrategy="kmeans").factorize()
    for strategy, name in (("sivm", "SIVM"), ("laesa", "LAESA")):
        with pytest.raises(ValueError, match=r"'%s' takes nsub <= 64 \(%s" % (strategy, name)):
            pymf_amd.SUB(sc.sub_data(4, 200), pymf_amd.NMF, nsub=65, sstrategy=strategy).factorize()
    with pytest.raises(ValueError, match="at most 16384 rows"):
        pymf_amd.SUB(np.ones((16385, 3), dtype=np.float32), pymf_amd.NMF, nsub=2, sstrategy="sivm").factorize()


def test_sparse_data_are_refused_before_any_device_call(no_device):
    sp = pytest.importorskip("scipy.sparse")
    S = sp.random(6, 40, density=0.3, format="csr", random_state=1, dtype=np.float32)
    with pytest.raises(TypeError, match="scipy.sparse data is not supported"):
        pymf_amd.SUB(S, pymf_amd.NMF, nsub=4).factorize()


def test_hull_is_refused_by_update_w_not_by_the_constructor(no_device):
    mdl = pymf_amd.SUB(data(), pymf_amd.NMF, sstrategy="hull")
    with pytest.raises(NotImplementedError, match="CHNMF"):
        mdl.update_w()
    with pytest.raises(NotImplementedError, match="'hull'"):
        mdl.factorize()


def test_rand_draws_what_the_reference_draws(no_device):
    V = data(6, 40)
    mdl = pymf_amd.SUB(V, pymf_amd.NMF, nsub=7)
    random.seed(12)
    got = mdl.randselect()
    nxt = random.random()
    random.seed(12)
    want = np.sort(np.int32(random.sample(range(40), 7)))                         # sub.py:160-161, range for xrange
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert nxt == random.random()                                                 # ... and nothing more of the stream


def test_cur_consumes_nsub_draws_and_returns_the_searchsorted_indices(fake):
    V = data(6, 40)
    Ctx.norms = np.random.RandomState(5).random_sample(40) + 0.01
    mdl = pymf_amd.SUB(V, pymf_amd.NMF, nsub=9, sstrategy="cur")
    np.random.seed(31)
    got = mdl.curselect()
    after = np.random.rand()
    np.random.seed(31)
    draws = np.array([np.random.rand() for _ in range(9)])
    assert after == np.random.rand()                                               # exactly nsub values of the stream
    cum = np.cumsum(Ctx.norms / Ctx.norms.sum())
    assert np.array_equal(got, np.sort(np.searchsorted(cum, draws, side="left")))
    assert np.array_equal(got, np.sort([np.where(cum >= r)[0][0] for r in draws]))   # sub.py:137-141
    # the norms came from a CUR context that was given the data once, from the host
    kinds = [e[0] for e in fake]
    assert kinds == ["set_v_dense", "cur_sqnorms"] and fake[0][1].algo == _lib.ALGO_CUR and fake[0][2].shape == V.shape
    # a draw beyond the last cumulative value is the last column (the reference: IndexError)
    Ctx.norms = np.array([1.0, 1e-30, 0.0])
    tail = pymf_amd.SUB(V[:, :3], pymf_amd.NMF, nsub=4, sstrategy="cur")
    real, calls = np.random.rand, []
    try:
        np.random.rand = lambda: (calls.append(1), 1.0 + 1e-12)[1]
        assert np.array_equal(tail.curselect(), [2, 2, 2, 2]) and len(calls) == 4
    finally:
        np.random.rand = real


def test_one_upload_per_call_with_stand_in_models(fake):
    """'rand': the full model is filled from the host and the sample gathered from it; the next call asks the model that holds
    the data, whose digest is unchanged, and fills both new models on the device; an in-place edit sends the data up once."""
    class Model(pymf_amd.NMF):
        def factorize(self, niter=1, compute_w=True, **kw):
            if compute_w:
                self.W = np.full((self._data_dimension, self._num_bases), float(self._num_samples))
            self.H = np.zeros((self._num_bases, self._num_samples))

        def frobenius_norm(self):
            return 1.25

    V = data(6, 40)
    mdl = pymf_amd.SUB(V, Model, nsub=7, num_bases=2, show_progress=False)
    random.seed(3)
    mdl.factorize()
    random.seed(3)
    idx = np.sort(np.int32(random.sample(range(40), 7)))
    assert [e[0] for e in fake] == ["set_v_dense", "set_v_gather"]
    full, small = fake[0][1], fake[1][1]
    assert (full.m, full.n, small.m, small.n) == (6, 40, 6, 7) and fake[1][2] is full and np.array_equal(fake[1][3], idx)
    assert np.array_equal(fake[0][2], V)
    assert isinstance(mdl.mdl, Model) and mdl.mdl.data is V
    assert np.array_equal(mdl.W, np.full((6, 2), 7.0)) and mdl.H.shape == (2, 40) and mdl.ferr.shape == (1,) and mdl.ferr[0] == 1.25
    del fake[:]
    mdl.factorize()                                                               # unchanged data: nothing crosses the host link
    assert [e[0] for e in fake] == ["set_v_gather", "set_v_gather"]
    assert fake[0][2] is full and fake[0][3] is None and fake[0][1].n == 40       # the new full model: a whole copy of the old one
    assert fake[1][2] is full and fake[1][1].n == 7
    new_full = fake[0][1]
    del fake[:]
    V[2, 5] += 1.0                                                                # an in-place edit
    mdl.factorize()
    assert [e[0] for e in fake] == ["set_v_dense", "set_v_gather", "set_v_gather"]
    assert fake[0][1] is new_full and np.array_equal(fake[0][2], V)               # the holder of the data is refreshed, once


def test_the_c_abi_entries_are_declared_bound_documented_and_exported():
    header = open(os.path.join(ROOT, "include", "pymf_hip.h")).read()
    assert re.search(r"int\s+pmf_set_v_gather_f32\(pmf_ctx\*\s*dst,\s*pmf_ctx\*\s*src,\s*const int64_t\*\s*idx,\s*int64_t\s+nsel\);", header)
    assert re.search(r"int\s+pmf_get_v_dense_f32\(pmf_ctx\*\s*ctx,\s*float\*\s*out,\s*int64_t\s+ld\);", header)
    bound = [s[0] for s in _lib.SYMBOLS]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("pmf_set_v_gather_f32", "pmf_get_v_dense_f32"):
        assert name in bound and name in doc
    lib = _lib.load()                                                             # every declared symbol is in the library
    assert hasattr(lib, "pmf_set_v_gather_f32") and hasattr(lib, "pmf_get_v_dense_f32")
    for name in ("set_v_gather", "get_v_dense"):
        assert hasattr(_lib.Context, name)
    api = open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_api.hip")).read()
    assert '#include "pmf_gather.h"' in api and '#include "pmf_host_gather.h"' in api
    assert "3.30" in open(os.path.join(ROOT, "DESIGN.md")).read()
