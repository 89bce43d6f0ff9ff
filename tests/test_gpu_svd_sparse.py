"""pymf_amd.SVD / PCA on scipy.sparse data (accept_sparse = True) on the MI355X against the float64 oracle on toarray(), cut at k
(tests/svd_oracle.py on the cases of tests/svd_sparse_cases.py), and against the dense device run on toarray().  S within 1e-9
relative (the dense path's bound); U, V, W, H, the orthonormality of the projected side and ferr^2 / ||data||^2 within 4 x the
deviation of the NumPy twin from the oracle (tests/golden/svd_sparse_tolerances.json; vectors floored at 1e-13, ferr^2 at
64 * 2^-52); the eigenvector side orthonormal to 1e-10; empty lines exactly 0; every repetition bit-equal."""
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import svd_cases as dc
import svd_oracle as so
import svd_sparse_cases as sc
import pymf_amd
from conftest import LEDGER_PATH, Measured
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

S_RTOL = 1e-9
_parity = {}


def within(value, tol, what):
    print("%-40s %.3e  (tol %.3e)" % (what, value, tol))
    _parity[what] = float(value)
    m = Measured(value)
    m.what = what
    return m <= tol


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    try:
        out = os.path.dirname(LEDGER_PATH)                    # beside the session's ledger; committed as profiles/parity_svd_sparse.json
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_svd_sparse.json"), "w") as f:
            json.dump({"achieved": _parity}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def run_svd(data, k, sparse=True):
    mdl = pymf_amd.SVD(data, k=k)
    mdl.accept_sparse = sparse
    mdl.factorize()
    return mdl


_runs = {}


def sparse_run(name):
    if name not in _runs:
        _runs[name] = run_svd(sc.sparse_data(name), sc.SVD_CASES[name]["k"])
    return sc.svd_case(name), _runs[name]


@pytest.mark.parametrize("name", sorted(sc.SVD_CASES))
def test_svd_against_the_oracle(name):
    c, mdl = sparse_run(name)
    rows, cols = c["data"].shape
    r = c["S"].shape[0]
    for a, shape in ((mdl.U, (rows, r)), (mdl.S, (r, r)), (mdl.V, (r, cols))):
        assert type(a) is np.ndarray and a.dtype == np.float64 and a.shape == shape
    assert np.array_equal(mdl.S, np.diag(np.diag(mdl.S)))
    s_np = np.linalg.svd(c["data"].astype(np.float64), compute_uv=False)[:r]
    assert within(float(np.max(np.abs(np.diag(mdl.S) - s_np) / s_np)), S_RTOL, name + " S vs numpy.linalg.svd")
    d = sc.svd_deviation(c, (mdl.U, mdl.S, mdl.V))
    ok = [within(d[q], sc.device_tol(q), "%s %s" % (name, q)) for q in ("U", "V", "orth_proj")]
    ok.append(within(d["S"], S_RTOL, name + " S"))
    eig_side = sc.orth(mdl.V, 1) if c["left"] else sc.orth(mdl.U, 0)
    ok.append(within(eig_side, 1e-10, name + " orthonormality of the eigenvector side"))
    got2 = mdl.frobenius_norm() ** 2 / float(np.sum(c["data"].astype(np.float64) ** 2))
    ok.append(within(abs(got2 - c["ferr2"]), sc.device_tol("ferr2"), name + " ferr2"))
    assert all(ok)
    # rows of U / columns of V that belong to empty lines are exactly 0
    assert np.all(mdl.U[np.count_nonzero(c["data"], axis=1) == 0] == 0.0)
    assert np.all(mdl.V[:, np.count_nonzero(c["data"], axis=0) == 0] == 0.0)


@pytest.mark.parametrize("name", sorted(sc.SVD_CASES))
def test_svd_against_the_dense_device_run(name):
    c, mdl = sparse_run(name)
    r = c["S"].shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dense = run_svd(c["data"], -1, sparse=False)
    assert dense.S.shape[0] >= r
    got = so.fix_svd_signs(mdl.U, mdl.V, c["left"])
    want = so.fix_svd_signs(dense.U[:, :r], dense.V[:r], c["left"])
    ok = [within(sc.max_abs(got[0], want[0]), dc.device_tol("U") + sc.device_tol("U"), name + " U vs dense run"),
          within(sc.max_abs(got[1], want[1]), dc.device_tol("V") + sc.device_tol("V"), name + " V vs dense run"),
          within(float(np.max(np.abs(np.diag(mdl.S) - np.diag(dense.S)[:r]) / np.diag(mdl.S))), 2 * S_RTOL, name + " S vs dense run")]
    assert all(ok)


def bits(mdl):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (mdl.U, mdl.S, mdl.V))


@pytest.mark.parametrize("name", sorted(sc.SVD_CASES))
def test_two_runs_and_a_second_factorize_give_the_same_bits(name):
    c, first = sparse_run(name)
    again = run_svd(sc.sparse_data(name), c["k"])
    assert bits(again) == bits(first)
    f1 = again.frobenius_norm()
    again.factorize()                                          # a second factorize() on the same object
    assert bits(again) == bits(first) and again.frobenius_norm() == f1 == first.frobenius_norm()


def test_formats_and_k_give_the_same_bits():
    # the three input formats of one case
    c, ref = sparse_run(sc.FORMATS_CASE)
    for fmt in ("csc", "coo_dup"):
        assert bits(run_svd(sc.sparse_data(sc.FORMATS_CASE, fmt), c["k"])) == bits(ref), fmt
    # k >= short - 1 and k = -1 keep every triple
    short = min(c["data"].shape)
    for k in (short - 1, short, 10 * short, 0):
        assert bits(run_svd(sc.sparse_data(sc.SAME_K_CASE), k)) == bits(ref), k
    # a float64 matrix warns once per object
    V64 = sc.sparse_data(sc.FORMATS_CASE).astype(np.float64)
    mdl = pymf_amd.SVD(V64)
    mdl.accept_sparse = True
    with pytest.warns(pymf_amd.nmf.PrecisionWarning):
        mdl.factorize()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mdl.factorize()
    assert bits(mdl) == bits(ref)


def run_pca(name, hooks=False):
    c = sc.pca_case(name)
    mdl = pymf_amd.PCA(sc.sparse_data(sc.PCA_CASES[name]["data"]), num_bases=c["num_bases"], center_mean=False)
    mdl.accept_sparse = True
    if c["user_w"] is not None:
        mdl.W = c["user_w"].copy()
    if hooks:
        if c["user_w"] is None:
            mdl.update_w()
        mdl.update_h()
        mdl.ferr = np.array([mdl.frobenius_norm()])
    else:
        mdl.factorize(compute_w=c["user_w"] is None)
    return c, mdl


@pytest.mark.parametrize("name", sorted(sc.PCA_CASES))
def test_pca_against_the_oracle(name):
    c, mdl = run_pca(name)
    ora = c["oracle"]
    assert mdl.W.dtype == np.float64 and mdl.H.dtype == np.float64
    assert mdl.W.shape == ora["W"].shape and mdl.H.shape == ora["H"].shape
    n2 = float(np.sum(c["data"].astype(np.float64) ** 2))
    got = dict(W=mdl.W, H=mdl.H, eigenvalues=None if c["user_w"] is not None else mdl.eigenvalues, ferr2=mdl.ferr[0] ** 2 / n2)
    d = sc.pca_deviation(c, got)
    ok = [within(d[q], sc.device_tol(q), "%s %s" % (name, q)) for q in ("W", "H", "pca_ferr2")]
    if "eigenvalues" in d:
        ok.append(within(d["eigenvalues"], S_RTOL, name + " eigenvalues"))
    assert all(ok)
    assert within(abs(mdl.frobenius_norm() ** 2 / n2 - ora["ferr2"]), sc.device_tol("pca_ferr2"), name + " frobenius_norm")
    # the hooks by hand equal factorize(); so does a second factorize() on the same object
    _, byhand = run_pca(name, hooks=True)
    assert byhand.W.tobytes() == mdl.W.tobytes() and byhand.H.tobytes() == mdl.H.tobytes() and byhand.ferr[0] == mdl.ferr[0]
    w, h, f = mdl.W.tobytes(), mdl.H.tobytes(), mdl.ferr[0]
    mdl.factorize(compute_w=c["user_w"] is None)
    assert mdl.W.tobytes() == w and mdl.H.tobytes() == h and mdl.ferr[0] == f


def test_the_c_abi_alone():
    c = sc.svd_case("29x300")
    A = sp.csr_matrix(c["data"])
    ctx = _lib.Context(_lib.ALGO_PCA, 29, 300, 29)
    try:
        assert ctx.path_name == "svd_gram_f64"
        # refused arrays never reach the device: unsorted columns, an index out of range
        bad = A.indices.copy()
        bad[:2] = bad[:2][::-1]
        for indices, why in ((bad, "ascend"), (np.where(np.arange(A.nnz) == 3, 300, A.indices), "out of range")):
            with pytest.raises(_lib.PmfError, match=why) as e:
                ctx.set_v_csr(A.indptr, indices, A.data)
            assert e.value.code == _lib.PMF_EINVAL and ctx.path_name == "svd_gram_f64"
        ctx.set_option("svd_num_triples", 7)
        ctx.set_v_csr(A.indptr, A.indices, A.data)
        assert ctx.path_name == "svd_csr"
        assert ctx.svd_decompose() == 7 and ctx.svd_rank() == 7
        U, S, V = ctx.svd_get(7)
        assert within(float(np.max(np.abs(S - np.diag(c["S"])[:7]) / S)), S_RTOL, "ABI S")
        f2 = ctx.frobenius() ** 2
        assert within(abs(f2 - float(np.sum(np.diag(c["S"])[7:] ** 2))) / float(np.sum(c["data"].astype(np.float64) ** 2)),
                      sc.device_tol("ferr2"), "ABI ferr2")
        for call in (lambda: ctx.stream_begin(), lambda: ctx.nndsvd_init(), lambda: ctx.fill_w_uniform(1)):
            with pytest.raises(_lib.PmfError, match="not while CSR data is resident on a PCA / SVD context") as e:
                call()
            assert e.value.code == _lib.PMF_EINVAL
        ctx.set_option("svd_num_triples", 0)
        assert ctx.svd_decompose() == 29
        # dense data brings the dense path back
        ctx.set_v_dense(c["data"])
        assert ctx.path_name == "svd_gram_f64"
        assert ctx.svd_decompose() == 29
        Ud, Sd, Vd = ctx.svd_get(29)
        assert within(float(np.max(np.abs(Sd - np.diag(c["S"])) / Sd)), S_RTOL, "ABI S dense again")
        assert ctx.frobenius() < 1e-3
    finally:
        ctx.close()


def test_a_tall_context_on_csr_data_holds_no_buffer_of_the_dense_image_s_size():
    """1 048 576 x 1 024: the dense image is 4 GiB, and the float32 W and its two scratch arrays are 4 GiB each at the context's
    width of 1 024.  They belong to dense data: with CSR data alone the context stays below 2 GiB (the row-count independent
    buffers, the CSR arrays, nothing else); the first dense upload allocates them."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    rows, cols = 1 << 20, 1 << 10
    A = sp.csr_matrix((np.ones(cols, dtype=np.float32), (np.arange(cols) * 1024, np.arange(cols))), shape=(rows, cols))
    warm = _lib.Context(_lib.ALGO_PCA, 64, 64, 64)             # (the runtime's own first allocations are not the context's)
    before = free_bytes()
    ctx = _lib.Context(_lib.ALGO_PCA, rows, cols, cols)
    try:
        ctx.set_v_csr(A.indptr, A.indices, A.data)
        assert ctx.path_name == "svd_csr"
        used = before - free_bytes()
        print("device memory of the context on CSR data: %.2f GiB" % (used / 2.0 ** 30))
        assert used < 2 << 30
    finally:
        ctx.close()
        warm.close()
