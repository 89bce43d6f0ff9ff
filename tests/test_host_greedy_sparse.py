"""GREEDY on scipy.sparse data without a GPU: the opt-in flag, the refusals that stay, the limits, the conversion that the class
hands to the device, the documents and the new kernels in the built library."""
import os
import sys

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib
from pymf_amd.greedycur import GREEDYCUR

sp = pytest.importorskip("scipy.sparse")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder(object):
    """A context that takes set_v_csr and nothing else."""
    k = 3

    def __init__(self):
        self.calls = []

    def set_v_csr(self, indptr, indices, vals):
        self.calls.append((np.array(indptr), np.array(indices), np.array(vals)))

    def update_w(self):
        raise StopIteration

    def __getattr__(self, name):
        raise AssertionError("device call: %s" % name)


def data(fmt="csr", dtype=np.float32, shape=(20, 10)):
    return sp.random(shape[0], shape[1], density=0.3, format=fmt, random_state=1, dtype=dtype)


def test_the_flag_is_a_class_attribute_and_off_by_default():
    assert pymf_amd.GREEDY.accept_sparse is False and pymf_amd.GREEDY._TAKES_SPARSE is True and GREEDYCUR._TAKES_SPARSE is False
    mdl = pymf_amd.GREEDY(data(), num_bases=2)
    for call in (mdl.factorize, mdl.update_w, mdl.update_h, mdl.frobenius_norm):
        with pytest.raises(TypeError, match=r"GREEDY: scipy.sparse data is not supported \(dense data only\)"):
            call()


def test_greedycur_refuses_with_the_flag_set():
    mdl = GREEDYCUR(data(), rrank=2)
    mdl.accept_sparse = True
    with pytest.raises(TypeError):
        mdl.factorize()


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_the_upload_hands_over_canonical_csr(fmt):
    V = data(fmt, np.float64)
    if fmt == "coo":                                           # duplicates: they add up
        V = sp.coo_matrix((np.concatenate([V.data, V.data[:5]]), (np.concatenate([V.row, V.row[:5]]), np.concatenate([V.col, V.col[:5]]))),
                          shape=V.shape)
    before = (V.data.copy(), V.nnz)
    mdl = pymf_amd.GREEDY(V, num_bases=3)
    mdl.accept_sparse = True
    mdl._ctx = ctx = Recorder()
    with pytest.warns(pymf_amd.nmf.PrecisionWarning):
        with pytest.raises(StopIteration):
            mdl.update_w()
    assert len(ctx.calls) == 1
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
    mdl = pymf_amd.GREEDY(V, num_bases=3)
    mdl.accept_sparse = True
    mdl._ctx = ctx = Recorder()
    with pytest.raises(StopIteration):
        mdl.update_w()
    assert ctx.calls[0][2].shape[0] == V.nnz and ctx.calls[0][2][3] == 0.0


def test_the_limits_are_refused_before_any_context(monkeypatch):
    def no_context(self):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(pymf_amd.GREEDY, "_context", no_context)

    def sparse_mdl(V, **kw):
        mdl = pymf_amd.GREEDY(V, **kw)
        mdl.accept_sparse = True
        return mdl

    wide = sp.random(1025, 1100, density=0.001, format="csr", random_state=3, dtype=np.float32)
    for call in ("factorize", "update_w", "update_h", "frobenius_norm"):
        with pytest.raises(ValueError, match="1024"):
            getattr(sparse_mdl(wide, num_bases=3), call)()
    with pytest.raises(ValueError, match="num_bases"):
        sparse_mdl(sp.random(8, 100, density=0.5, format="csr", random_state=3, dtype=np.float32), num_bases=65).factorize()
    mdl = sparse_mdl(data(), num_bases=2)
    mdl.stream_rows = 64                                       # resident data only
    with pytest.raises(ValueError, match="stream_rows"):
        mdl.factorize()

    class World(object):
        size, rank, local_rank = 2, 0, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    with pytest.raises(NotImplementedError):
        sparse_mdl(data(), num_bases=2).factorize()


def test_frobenius_norm_without_factors_is_the_sentinel_of_the_base_class():
    mdl = pymf_amd.GREEDY(data(), num_bases=2)
    mdl.accept_sparse = True
    assert mdl.frobenius_norm() == -123456                     # no W, no H: nmf.py:100-114, whatever the data


def test_the_documents():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert "greedy_csr" in header and "k_greedy_csr_pass" in header and "k_greedy_step_csr" in header
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "greedy_csr" in f.read()
    for sym in ("pmf_set_v_csr_f32", "pmf_greedy_select", "pmf_sivm_get_select", "pmf_update_w", "pmf_update_h", "pmf_frobenius", "pmf_factorize"):
        assert sym in [s[0] for s in _lib.SYMBOLS]
    _lib.load()                                                # every declared symbol is in the library
    assert "accept_sparse" in pymf_amd.greedy.__doc__ and "ARPACK" in pymf_amd.greedy.__doc__


def test_the_new_kernels_are_in_the_built_library_without_a_private_segment():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf of the ROCm image is not here")
    rows = {r["dem"]: r for r in kernel_regs.kernels(_lib.LIB_PATH)}
    for name in ("k_greedy_csr_pass<1>", "k_greedy_csr_pass<2>", "k_greedy_step_csr", "k_greedy_step", "k_greedy_csr_gather", "k_greedy_csr_pinv_t",
                 "k_greedy_csr_widen", "k_greedy_csr_ht"):
        r = next(v for key, v in rows.items() if key == name or key.startswith(name + "("))
        assert int(r["scratch"]) == 0 and int(r["wg"]) == 256, r
    for cpl in (1, 2):                                         # the pass keeps no LDS beyond the reduce and at least four waves per SIMD
        r = next(v for key, v in rows.items() if key.startswith("k_greedy_csr_pass<%d>" % cpl))
        assert int(r["lds"]) <= 64 and int(r["vgpr"]) <= 128, r
