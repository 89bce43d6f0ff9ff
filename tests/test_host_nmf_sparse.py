"""CPU-side checks of NMF on scipy.sparse data (NMF.accept_sparse): the flag's default and the unchanged refusal, the classes
that keep refusing whatever the flag says, compute_err, frobenius_norm and the limits -- all decided on the host, before any
device call.  No GPU needed: the context is a stand-in that fails the test when anything but the expected call reaches it."""
import numpy as np
import pytest

import pymf_amd
from pymf_amd.rnmf import RNMF

sp = pytest.importorskip("scipy.sparse")
CLASSES = {"BNMF": pymf_amd.BNMF, "RNMF": RNMF, "NMFALS": pymf_amd.NMFALS, "NMFNNLS": pymf_amd.NMFNNLS, "CNMF": pymf_amd.CNMF}


class NoDevice(object):
    """A context nobody may touch."""

    def __getattr__(self, name):
        raise AssertionError("device call: %s" % name)


class NoData(object):
    """A context that takes settings (BNMF's and RNMF's lambda) but no data, no step and no loop."""

    def __getattr__(self, name):
        if name.startswith("set_v") or name.startswith("update") or name.startswith("factorize") or name.startswith("stream"):
            raise AssertionError("device call: %s" % name)
        return lambda *a, **kw: None


class Recorder(object):
    """A context that takes set_v_csr and nothing else."""

    def __init__(self):
        self.calls = []

    def set_v_csr(self, indptr, indices, vals):
        self.calls.append((np.array(indptr), np.array(indices), np.array(vals)))

    def __getattr__(self, name):
        raise AssertionError("device call: %s" % name)


def data(fmt="csr", dtype=np.float32):
    return sp.random(20, 10, density=0.3, format=fmt, random_state=1, dtype=dtype)


def test_the_flag_defaults_to_false_on_every_class():
    assert pymf_amd.NMF.accept_sparse is False
    for name, cls in list(CLASSES.items()) + [("SNMF", pymf_amd.SNMF)]:
        assert cls.accept_sparse is False, name


def test_without_the_flag_sparse_data_raise_the_same_type_error(monkeypatch):
    monkeypatch.setattr(pymf_amd.NMF, "_context", lambda self: NoDevice())
    mdl = pymf_amd.NMF(data(), num_bases=2)
    with pytest.raises(TypeError, match=r"scipy.sparse data is not supported by NMF \(the reference fails with UFuncTypeError"):
        mdl.factorize(niter=1, compute_err=False)
    with pytest.raises(TypeError, match="not supported by NMF"):
        mdl.factorize(niter=1)                                 # compute_err=True: still the refusal of the data


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_other_classes_refuse_sparse_data_whatever_the_flag(monkeypatch, name):
    monkeypatch.setattr(pymf_amd.NMF, "_context", lambda self: NoData())
    for kw in (dict(compute_err=False), dict()):               # (a fresh object each: RNMF's failed init_h leaves an H without S)
        mdl = CLASSES[name](data(), num_bases=2)
        mdl.accept_sparse = True
        with pytest.raises(TypeError):
            mdl.factorize(niter=1, **kw)


def test_compute_err_is_refused_before_any_device_call(monkeypatch):
    def no_context(self):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(pymf_amd.NMF, "_context", no_context)
    mdl = pymf_amd.NMF(data(), num_bases=2)
    mdl.accept_sparse = True
    with pytest.raises(TypeError, match="compute_err=True on scipy.sparse data"):
        mdl.factorize(niter=3)
    assert not mdl._has("W") and not mdl._has("H")             # ... and before the start is drawn
    # SNMF's wording, word for word
    snmf = pymf_amd.SNMF(data(), num_bases=2)
    with pytest.raises(TypeError) as e:
        snmf.factorize(niter=3)
    with pytest.raises(TypeError) as e2:
        mdl.factorize(niter=3)
    assert str(e.value) == str(e2.value)


def test_frobenius_norm_is_the_references_sentinel(monkeypatch):
    monkeypatch.setattr(pymf_amd.NMF, "_context", lambda self: NoDevice())
    mdl = pymf_amd.NMF(data(), num_bases=2)
    mdl.accept_sparse = True
    assert mdl.frobenius_norm() == -123456
    mdl.W, mdl.H = np.ones((20, 2)), np.ones((2, 10))
    assert mdl.frobenius_norm() == -123456


def test_a_subclass_that_overrides_hooks_is_taken(monkeypatch):
    class Mine(pymf_amd.NMF):
        accept_sparse = True

        def update_h(self):
            pymf_amd.NMF.update_h(self)

    ctx = Recorder()
    mdl = Mine(data(), num_bases=2)
    assert mdl._sparse_nmf()
    mdl._upload_data(ctx)
    assert len(ctx.calls) == 1


@pytest.mark.parametrize("fmt", ["csr", "coo", "csc"])
def test_the_upload_hands_over_canonical_csr_and_warns_once_for_float64(fmt):
    V = data(fmt, np.float64)
    mdl = pymf_amd.NMF(V, num_bases=2)
    mdl.accept_sparse = True
    ctx = Recorder()
    with pytest.warns(pymf_amd.nmf.PrecisionWarning) as rec:
        mdl._upload_data(ctx)
        mdl._v_src = None
        mdl._upload_data(ctx)                                  # a second upload: no second warning
    assert len([w for w in rec if issubclass(w.category, pymf_amd.nmf.PrecisionWarning)]) == 1
    assert len(ctx.calls) == 2
    indptr, indices, vals = ctx.calls[0]
    ref = V.tocsr()
    ref.sum_duplicates()
    assert np.array_equal(indptr, ref.indptr) and np.array_equal(indices, ref.indices) and np.array_equal(vals, ref.data)


def test_unsummed_duplicates_are_summed_on_a_copy():
    indptr = np.array([0, 2, 3], dtype=np.int32)
    indices = np.array([1, 1, 0], dtype=np.int32)
    vals = np.array([1.0, 2.0, 5.0], dtype=np.float32)
    V = sp.csr_matrix((vals, indices, indptr), shape=(2, 3))
    mdl = pymf_amd.NMF(V, num_bases=1)
    mdl.accept_sparse = True
    ctx = Recorder()
    mdl._upload_data(ctx)
    assert ctx.calls[0][2].tolist() == [3.0, 5.0] and ctx.calls[0][1].tolist() == [1, 0]
    assert V.nnz == 3 and V.data.tolist() == [1.0, 2.0, 5.0]   # the caller's matrix keeps its entries


def test_the_limits_are_named_on_the_host(monkeypatch):
    mdl = pymf_amd.NMF(sp.random(200, 150, density=0.1, format="csr", random_state=2, dtype=np.float32), num_bases=129)
    mdl.accept_sparse = True
    with pytest.raises(ValueError, match="num_bases > 128"):
        mdl._upload_data(NoDevice())

    class World(object):
        size, rank = 2, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    mdl = pymf_amd.NMF(data(), num_bases=2)
    mdl.accept_sparse = True
    with pytest.raises(NotImplementedError, match="one rank"):
        mdl._upload_data(NoDevice())
