"""pymf_amd.LAESA and pymf_amd.GMAP without a GPU: the exports, the constructors, the documented options, the refusals."""
import os

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])


def test_exports_and_the_shared_algorithm_number():
    for name in ("LAESA", "GMAP"):
        assert name in pymf_amd.__all__
        cls = getattr(pymf_amd, name)
        assert issubclass(cls, pymf_amd.SIVM)
        assert cls._ALGO == _lib.ALGO_SIVM == 10          # no algorithm number of their own
        assert cls._NITER == 1


def test_the_header_documents_the_options_and_the_reference_mappings():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    for word in ('"sivm_rule"', '"gmap_method"', "laesa.py", "gmap.py", "robust_map"):
        assert word in header, word


def test_constructor_defaults_and_zero_initialisations():
    mdl = pymf_amd.LAESA(DOC)
    assert (mdl._num_bases, mdl._dist_measure, mdl._init) == (4, "l2", "fastmap")
    g = pymf_amd.GMAP(DOC)
    assert (g._num_bases, g._method, g._robust_map, g.sub) == (4, "pca", True, [])
    for m in (mdl, g):
        m.init_w()
        m.init_h()
        assert np.array_equal(m.W, np.zeros((2, 4))) and np.array_equal(m.H, np.zeros((4, 3)))


def test_the_doc_examples_are_accepted():
    """laesa.py:47-59 and gmap.py:58-70: the signatures, up to the point where a device would be needed."""
    pymf_amd.LAESA(DOC, num_bases=2)._check_supported()
    mdl = pymf_amd.LAESA(np.array([[1.5, 1.3], [1.2, 0.3]]), num_bases=2)
    mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    mdl._check_supported()
    import inspect
    assert list(inspect.signature(pymf_amd.LAESA.factorize).parameters) == ["self", "show_progress", "compute_w", "compute_h", "compute_err", "niter"]
    assert list(inspect.signature(pymf_amd.GMAP.factorize).parameters) == ["self", "show_progress", "compute_w", "compute_h", "compute_err",
                                                                           "robust_cluster", "niter", "robust_nselect"]
    assert list(inspect.signature(pymf_amd.GMAP.__init__).parameters) == ["self", "data", "num_bases", "method", "robust_map"]
    pymf_amd.GMAP(DOC, num_bases=2, robust_map=False)._check_supported()
    for method in ("pca", "aa", "nmf"):
        pymf_amd.GMAP(DOC, num_bases=2, method=method, robust_map=False)._check_supported()


def test_gmap_robust_map_is_refused_by_every_entry_point():
    mdl = pymf_amd.GMAP(DOC, num_bases=2)                     # the reference's default: robust_map=True
    mdl.W = np.eye(2)
    mdl.H = np.zeros((2, 3))
    for call in (mdl.factorize, mdl.update_w, mdl.update_h, mdl.frobenius_norm):
        with pytest.raises(NotImplementedError, match="robust_map=False"):
            call()


def test_gmap_bad_method():
    mdl = pymf_amd.GMAP(DOC, num_bases=2, method="ica", robust_map=False)
    for call in (mdl.factorize, mdl.update_w):
        with pytest.raises(ValueError, match="method"):
            call()


@pytest.mark.parametrize("cls,kw", [(pymf_amd.LAESA, {}), (pymf_amd.GMAP, {"robust_map": False})])
def test_sivms_refusals_are_inherited(cls, kw):
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(TypeError):
        cls(sp.csr_matrix(np.ones((3, 5))), num_bases=2, **kw)._check_supported()
    mdl = cls(np.ones((3, 5)), num_bases=2, **kw)
    mdl.stream_rows = 64
    with pytest.raises(ValueError):
        mdl._check_supported()
    with pytest.raises(ValueError):
        cls(np.ones((3, 100)), num_bases=65, **kw)._check_supported()
    if cls is pymf_amd.LAESA:
        with pytest.raises(NotImplementedError):
            cls(np.ones((3, 5)), num_bases=2, dist_measure="kl")._check_supported()
        with pytest.raises(ValueError):
            cls(np.ones((3, 5)), num_bases=2, init="random")._check_supported()
