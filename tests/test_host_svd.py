"""pymf_amd.SVD / PCA without a GPU: exports, constructor attributes, centring, refusals, the niter override."""
import os
import re
import warnings

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])


def test_exports_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_svd_decompose\(pmf_ctx\*\s*ctx,\s*int32_t\*\s*rank\);", header)
    assert re.search(r"int\s+pmf_svd_get\(pmf_ctx\*\s*ctx,\s*double\*\s*U,\s*double\*\s*S,\s*double\*\s*V\);", header)
    assert "PMF_ALGO_PCA = 12" in header
    bound = [s[0] for s in _lib.SYMBOLS]
    assert "pmf_svd_decompose" in bound and "pmf_svd_get" in bound and "pmf_svd_rank" in bound
    assert _lib.ALGO_PCA == 12
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "pmf_svd_decompose" in doc and "pmf_svd_get" in doc and "pmf_svd_rank" in doc
    assert "SVD" in pymf_amd.__all__ and "PCA" in pymf_amd.__all__


def test_algo_values_7_and_9_stay_refused():
    for algo in (7, 9, 13):
        with pytest.raises(_lib.PmfError) as ei:
            _lib.Context(algo, 4, 4, 2)
        assert ei.value.code == _lib.PMF_EINVAL


def test_context_limits():
    def code(*args):
        try:
            _lib.Context(*args).close()
        except _lib.PmfError as e:
            return e.code
        return _lib.PMF_OK
    assert code(_lib.ALGO_PCA, 2433, 3000, 2433) == _lib.PMF_EINVAL          # min(rows, cols) beyond the limit
    assert code(_lib.ALGO_PCA, 30, 40, 29) == _lib.PMF_EINVAL                # fewer bases than the largest possible rank
    ok = code(_lib.ALGO_PCA, 30, 40, 30)
    assert ok == (_lib.PMF_OK if _lib.device_count() > 0 else _lib.PMF_EHIP)


def test_svd_constructor_attributes():
    mdl = pymf_amd.SVD(DOC)
    assert (mdl._rows, mdl._cols, mdl._rrank, mdl._crank, mdl._k) == (2, 3, 2, 3, -1)
    assert mdl.data is DOC and pymf_amd.SVD._EPS == 1e-8
    mdl = pymf_amd.SVD(DOC, k=1, rrank=1, crank=2)
    assert (mdl._rrank, mdl._crank, mdl._k) == (1, 2, 1)
    with pytest.raises(AttributeError):
        mdl.frobenius_norm()                                   # no U yet, as in the reference


def test_pca_constructor_centres_like_the_reference():
    mdl = pymf_amd.PCA(DOC)
    assert mdl._num_bases == 0 and mdl._center_mean is True
    assert mdl._data_orig is DOC
    assert np.array_equal(mdl._meanv, DOC.mean(axis=1).reshape(2, 1))
    assert np.array_equal(mdl.data, DOC - DOC.mean(axis=1).reshape(2, 1))
    assert (mdl._data_dimension, mdl._num_samples) == (2, 3)
    raw = pymf_amd.PCA(DOC, num_bases=2, center_mean=False)
    assert raw.data is DOC and not hasattr(raw, "_data_orig") and raw._num_bases == 2
    f32 = pymf_amd.PCA(DOC.astype(np.float32))
    assert f32.data.dtype == np.float32
    assert pymf_amd.PCA._NITER == 1


def test_pca_inits_do_nothing():
    mdl = pymf_amd.PCA(DOC, num_bases=2)
    mdl.init_w()
    mdl.init_h()
    assert not mdl._has("W") and not mdl._has("H")
    with pytest.raises(AttributeError):
        mdl.update_h()                                         # no W, as the reference's self.W would raise


def test_refusals():
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(TypeError):
        pymf_amd.SVD(sp.csr_matrix(np.ones((3, 5)))).factorize()
    with pytest.raises(TypeError):
        pymf_amd.PCA(sp.csr_matrix(np.ones((3, 5))), num_bases=2).factorize()
    mdl = pymf_amd.PCA(np.ones((3, 5)), num_bases=2)
    mdl.stream_rows = 64
    for call in (mdl.factorize, mdl.update_w, mdl.frobenius_norm):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        pymf_amd.SVD(np.zeros((2433, 2433), dtype=np.float32)).factorize()
    with pytest.raises(ValueError):
        pymf_amd.PCA(np.ones((3, 5)), num_bases=2433).factorize()

    class World(object):
        size, rank = 2, 0

    mdl = pymf_amd.PCA(np.ones((3, 5)), num_bases=2)
    mdl._world = lambda: World()
    with pytest.raises(NotImplementedError):
        mdl.factorize()


def test_factorize_forces_one_iteration(monkeypatch):
    seen = {}

    def fake(self, niter=1, **kw):
        seen.update(kw, niter=niter)

    monkeypatch.setattr(pymf_amd.NMF, "factorize", fake)
    pymf_amd.PCA(DOC, num_bases=2).factorize(niter=7, compute_w=False)
    assert seen["niter"] == 1 and seen["compute_w"] is False and seen["compute_h"] is True


@pytest.mark.gpu
def test_float64_data_warns_once():
    mdl = pymf_amd.PCA(DOC, num_bases=2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        mdl.factorize()
        mdl.factorize()
    assert len([x for x in w if issubclass(x.category, pymf_amd.nmf.PrecisionWarning)]) == 1
    svd = pymf_amd.SVD(DOC)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        svd.factorize()
        svd.factorize()
    assert len([x for x in w if issubclass(x.category, pymf_amd.nmf.PrecisionWarning)]) == 1


@pytest.mark.gpu
def test_eigenvalues_are_singular_values():
    data = DOC.astype(np.float32)
    mdl = pymf_amd.PCA(data, num_bases=2, center_mean=False)
    mdl.factorize()
    assert np.allclose(mdl.eigenvalues, np.linalg.svd(DOC, compute_uv=False), rtol=1e-9, atol=0)
    assert mdl.W.dtype == np.float64 and mdl.H.dtype == np.float64 and mdl.W.shape == (2, 2) and mdl.H.shape == (2, 3)
