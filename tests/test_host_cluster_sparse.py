"""Kmeans and Cmeans on scipy.sparse data without a GPU: the opt-in flag, the refusals that stay, the conversion that the classes
hand to the device, the dense W of init_w, the documents and the new kernels in the built library."""
import os
import random
import sys

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

sp = pytest.importorskip("scipy.sparse")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["Kmeans", "Cmeans"]


class Recorder(object):
    """A context that takes set_v_csr and the factor uploads, and nothing else."""
    k = 3

    def __init__(self):
        self.calls = []
        self.dense = 0

    def set_v_csr(self, indptr, indices, vals):
        self.calls.append((np.array(indptr), np.array(indices), np.array(vals)))

    def set_v_dense(self, arr):
        self.dense += 1

    def set_w(self, W):
        pass

    def set_h(self, H):
        pass

    def update_h(self):
        raise StopIteration

    def __getattr__(self, name):
        raise AssertionError("device call: %s" % name)


def data(fmt="csr", dtype=np.float32, shape=(20, 10)):
    return sp.random(shape[0], shape[1], density=0.3, format=fmt, random_state=1, dtype=dtype)


def sparse_mdl(cls, V, **kw):
    mdl = getattr(pymf_amd, cls)(V, **kw)
    mdl.accept_sparse = True
    return mdl


@pytest.mark.parametrize("cls", CLASSES)
def test_the_flag_is_a_class_attribute_and_off_by_default(cls):
    assert getattr(pymf_amd, cls).accept_sparse is False
    mdl = getattr(pymf_amd, cls)(data(), num_bases=2)
    for call in (mdl.factorize, mdl.update_w, mdl.update_h, mdl.frobenius_norm):
        with pytest.raises(TypeError, match=r"%s: scipy.sparse data is not supported \(dense data only\)" % cls):
            call()


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_the_upload_hands_over_canonical_csr(cls, fmt):
    V = data(fmt, np.float64)
    if fmt == "coo":                                           # duplicates: they add up
        V = sp.coo_matrix((np.concatenate([V.data, V.data[:5]]), (np.concatenate([V.row, V.row[:5]]), np.concatenate([V.col, V.col[:5]]))),
                          shape=V.shape)
    before = (V.data.copy(), V.nnz)
    mdl = sparse_mdl(cls, V, num_bases=3)
    mdl.W = np.ones((20, 3))
    mdl.H = np.ones((3, 10))
    mdl._ctx = ctx = Recorder()
    with pytest.warns(pymf_amd.nmf.PrecisionWarning) as rec:
        with pytest.raises(StopIteration):
            mdl.update_h()
    assert len([w for w in rec if issubclass(w.category, pymf_amd.nmf.PrecisionWarning)]) == 1
    assert len(ctx.calls) == 1 and ctx.dense == 0              # never a dense upload
    indptr, indices, vals = ctx.calls[0]
    ref = V.tocsr()
    ref.sum_duplicates()
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and vals.dtype == np.float32
    assert np.array_equal(indptr, ref.indptr) and np.array_equal(indices, ref.indices)
    assert np.array_equal(vals, ref.data.astype(np.float32))
    _lib.check_csr(20, 10, indptr, indices)
    assert all(np.all(np.diff(indices[indptr[r]:indptr[r + 1]]) > 0) for r in range(20))
    assert V.nnz == before[1] and np.array_equal(V.data, before[0])            # the caller's matrix is untouched


def test_stored_zeros_are_kept():
    V = data().tocsr()
    V.data[3] = 0.0
    mdl = sparse_mdl("Cmeans", V, num_bases=3)
    mdl.W = np.ones((20, 3))
    mdl.H = np.ones((3, 10))
    mdl._ctx = ctx = Recorder()
    with pytest.raises(StopIteration):
        mdl.update_h()
    assert ctx.calls[0][2].shape[0] == V.nnz and ctx.calls[0][2][3] == 0.0


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_kmeans_init_w_binds_a_dense_w(fmt):
    V = data(fmt)
    mdl = sparse_mdl("Kmeans", V, num_bases=3)
    random.seed(4)
    mdl.init_w()
    random.seed(4)
    sel = sorted(random.sample(range(10), 3))
    assert type(mdl.W) is np.ndarray and mdl.W.shape == (20, 3)
    assert np.array_equal(mdl.W, V.toarray()[:, sel])


def test_cmeans_inits_draw_as_on_dense_data():
    mdl = sparse_mdl("Cmeans", data(), num_bases=3)
    np.random.seed(2)
    mdl.init_w()
    mdl.init_h()
    np.random.seed(2)
    assert np.array_equal(mdl.W, np.random.random((20, 3))) and np.array_equal(mdl.H, np.random.random((3, 10)))


@pytest.mark.parametrize("cls", CLASSES)
def test_the_other_refusals_are_unchanged(cls, monkeypatch):
    def no_context(self):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(getattr(pymf_amd, cls), "_context", no_context)
    with pytest.raises(ValueError, match="num_bases"):
        sparse_mdl(cls, data(shape=(8, 200)), num_bases=129).factorize()
    mdl = sparse_mdl(cls, data(), num_bases=2)
    mdl.stream_rows = 64                                       # resident data only
    with pytest.raises(ValueError, match="stream_rows"):
        mdl.factorize()

    class World(object):
        size, rank, local_rank = 2, 0, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    with pytest.raises(NotImplementedError):
        sparse_mdl(cls, data(), num_bases=2).factorize()


@pytest.mark.parametrize("cls", CLASSES)
def test_frobenius_norm_without_factors_is_the_sentinel_of_the_base_class(cls):
    assert sparse_mdl(cls, data(), num_bases=2).frobenius_norm() == -123456     # no W, no H: nmf.py:100-114, whatever the data


def test_the_documents():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert "cluster_csr" in header and "k_cluster_csr_assign" in header and "k_cluster_csr_num" in header
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "cluster_csr" in f.read()
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "3.27" in f.read()
    for sym in ("pmf_set_v_csr_f32", "pmf_cluster_get_assigned", "pmf_cluster_set_assigned", "pmf_update_w", "pmf_update_h", "pmf_frobenius",
                "pmf_factorize"):
        assert sym in [s[0] for s in _lib.SYMBOLS]
    _lib.load()                                                # every declared symbol is in the library
    assert "accept_sparse" in pymf_amd.kmeans.__doc__ and "accept_sparse" in pymf_amd.cmeans.__doc__


def test_the_new_kernels_are_in_the_built_library_without_a_private_segment():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf of the ROCm image is not here")
    rows = {r["dem"]: r for r in kernel_regs.kernels(_lib.LIB_PATH)}
    names = ["k_cluster_csr_%s<%d, %d>" % (stem, nh, algo) for stem in ("assign", "num", "den") for nh in (1, 2) for algo in (0, 1)]
    names += ["k_cluster_csr_finish<0>", "k_cluster_csr_finish<1>", "k_cluster_csr_wnorm", "k_cluster_csr_widen", "k_cluster_csr_ht"]
    for name in names:
        r = next(v for key, v in rows.items() if key == name or key.startswith(name + "("))
        assert int(r["scratch"]) == 0 and int(r["wg"]) == 256, r
    for nh in (1, 2):                                          # the H step keeps four waves per SIMD at least
        for algo in (0, 1):
            r = next(v for key, v in rows.items() if key.startswith("k_cluster_csr_assign<%d, %d>" % (nh, algo)))
            assert int(r["vgpr"]) <= 128, r
