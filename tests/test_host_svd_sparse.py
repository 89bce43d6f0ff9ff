"""SVD / PCA on scipy.sparse data without a GPU: the opt-in flag, the refusals that stay, the limits, the conversion that the
classes hand to the device, and the host-side check of CSR arrays."""
import os

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

sp = pytest.importorskip("scipy.sparse")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder(object):
    """A context that takes set_v_csr and set_option and nothing else."""
    k = 10

    def __init__(self):
        self.calls, self.options = [], {}

    def set_v_csr(self, indptr, indices, vals):
        self.calls.append((np.array(indptr), np.array(indices), np.array(vals)))

    def set_option(self, name, value):
        self.options[name] = value

    def svd_decompose(self):
        raise StopIteration

    def __getattr__(self, name):
        raise AssertionError("device call: %s" % name)


def data(fmt="csr", dtype=np.float32, shape=(20, 10)):
    return sp.random(shape[0], shape[1], density=0.3, format=fmt, random_state=1, dtype=dtype)


def test_the_flag_is_a_class_attribute_and_off_by_default():
    assert pymf_amd.SVD.accept_sparse is False and pymf_amd.PCA.accept_sparse is False
    with pytest.raises(TypeError, match=r"SVD: scipy.sparse data is not supported \(dense data only\)"):
        pymf_amd.SVD(data()).factorize()
    with pytest.raises(TypeError, match=r"PCA: scipy.sparse data is not supported \(dense data only\)"):
        pymf_amd.PCA(data(), num_bases=2, center_mean=False).factorize()
    mdl = pymf_amd.PCA(data(), num_bases=2, center_mean=False)
    for call in (mdl.update_w, mdl.update_h, mdl.frobenius_norm):
        with pytest.raises(TypeError):
            call()


def test_centred_pca_on_sparse_data_is_refused():
    mdl = pymf_amd.PCA(data(), num_bases=2)                    # center_mean=True: the constructor skips centring sparse input
    mdl.accept_sparse = True
    mdl.W = np.ones((20, 2))
    for call in (mdl.factorize, mdl.update_w, mdl.update_h, mdl.frobenius_norm):
        with pytest.raises(ValueError, match="center_mean=False") as e:
            call()
        assert isinstance(e.value, TypeError)                  # (what such data raised before the flag existed, too)


def test_the_limits_are_named(monkeypatch):
    wide = sp.random(1025, 1100, density=0.001, format="csr", random_state=3, dtype=np.float32)
    svd = pymf_amd.SVD(wide)
    svd.accept_sparse = True
    with pytest.raises(ValueError, match="1024"):
        svd.factorize()
    pca = pymf_amd.PCA(wide, num_bases=3, center_mean=False)
    pca.accept_sparse = True
    with pytest.raises(ValueError, match="1024"):
        pca.factorize()
    pca = pymf_amd.PCA(data(), num_bases=2, center_mean=False)
    pca.accept_sparse = True
    pca.stream_rows = 64                                       # resident data only: a sparse matrix is never streamed
    assert pca._stream_rows() == 0
    with pytest.raises(ValueError, match="stream_rows"):
        pca.factorize()

    class World(object):
        size, rank, local_rank = 2, 0, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    svd = pymf_amd.SVD(data())
    svd.accept_sparse = True
    with pytest.raises(ValueError, match="one rank"):
        svd.factorize()
    pca = pymf_amd.PCA(data(), num_bases=2, center_mean=False)
    pca.accept_sparse = True
    with pytest.raises(ValueError, match="one rank"):
        pca.factorize()


def test_pinv_and_cursl_keep_refusing(monkeypatch):
    monkeypatch.setattr(pymf_amd.SVD, "accept_sparse", True)   # the switch is per object: a value on the shared class changes nothing
    with pytest.raises(TypeError):
        pymf_amd.svd.pinv(data())
    with pytest.raises(TypeError):
        pymf_amd.SVD(data()).factorize()
    from pymf_amd.cursl import CURSL
    mdl = CURSL(data(), rrank=2)
    mdl.accept_sparse = True
    with pytest.raises(TypeError):
        mdl.factorize()


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_the_upload_hands_over_canonical_csr_and_k(fmt):
    V = data(fmt, np.float64)
    for k, want in ((-1, 0), (3, 3), (8, 8), (9, 0), (40, 0)):  # svd.py:165,204: 0 < k < short - 1 = 9
        mdl = pymf_amd.SVD(V, k=k)
        mdl.accept_sparse = True
        mdl._ctx = ctx = Recorder()
        with pytest.warns(pymf_amd.nmf.PrecisionWarning):
            with pytest.raises(StopIteration):
                mdl.factorize()
        assert ctx.options == {"svd_num_triples": want}
        indptr, indices, vals = ctx.calls[0]
        ref = V.tocsr()
        ref.sum_duplicates()
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and vals.dtype == np.float32
        assert np.array_equal(indptr, ref.indptr) and np.array_equal(indices, ref.indices)
        assert np.array_equal(vals, ref.data.astype(np.float32))
        _lib.check_csr(20, 10, indptr, indices)
        assert all(np.all(np.diff(indices[indptr[r]:indptr[r + 1]]) > 0) for r in range(20))


def test_frobenius_norm_wants_the_factors_of_the_last_call():
    class Ferr(Recorder):
        def frobenius(self):
            return 1.5

    mdl = pymf_amd.SVD(data())
    mdl.accept_sparse = True
    with pytest.raises(AttributeError):
        mdl.frobenius_norm()
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


def test_the_exports_and_the_documents():
    names = [s[0] for s in _lib.SYMBOLS]
    for sym in ("pmf_set_v_csr_f32", "pmf_svd_decompose", "pmf_svd_rank", "pmf_svd_get", "pmf_update_w", "pmf_update_h", "pmf_frobenius",
                "pmf_set_option", "pmf_path_name"):
        assert sym in names
    _lib.load()                                                # every declared symbol is in the library
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert "svd_num_triples" in header and "svd_csr" in header
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "svd_num_triples" in f.read()


def test_refused_csr_arrays_never_reach_the_device():
    """The arrays the device entry point refuses are refused by the host check it runs first (pmf_check_csr is that check,
    csr_check; the ascending order within a row on top of it is pinned on the device in tests/test_gpu_svd_sparse.py)."""
    indptr = np.array([0, 2, 3], dtype=np.int64)
    with pytest.raises(_lib.PmfError, match="column index out of range"):
        _lib.check_csr(2, 3, indptr, np.array([0, 3, 1], dtype=np.int32))
    with pytest.raises(_lib.PmfError, match="indptr"):
        _lib.check_csr(2, 3, np.array([0, 3, 2], dtype=np.int64), np.array([0, 1, 2], dtype=np.int32))
    _lib.check_csr(2, 3, indptr, np.array([2, 0, 1], dtype=np.int32))   # unsorted: well-formed for SNMF, refused on a PCA / SVD context
