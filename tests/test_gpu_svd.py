"""pymf_amd.SVD / PCA on the MI355X against the reference goldens and the float64 oracle (tests/svd_oracle.py) on the cases of
tests/svd_cases.py.  The singular values must equal numpy.linalg.svd of the float32 data to 1e-9 (the Gram matrix is float64:
only Jacobi's convergence stands between them); vectors, H and the errors within 4 x the deviation of the oracle's float32
twin (tests/golden/svd_tolerances.json), signs fixed on the eigenvector side."""
import warnings

import numpy as np
import pytest

import pymf_amd
import svd_cases as sc
import svd_oracle as so
from conftest import Measured, load_golden
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

S_RTOL = 1e-9
ORTHO_TOL = 1e-10


def measured(value, what):
    m = Measured(value)
    m.what = what
    return m


_runs = {}


def device_svd(name):
    if name not in _runs:
        c = sc.svd_case(name)
        mdl = pymf_amd.SVD(c["data"])
        mdl.factorize()
        _runs[name] = mdl
    return sc.svd_case(name), _runs[name]


@pytest.mark.parametrize("name", sorted(sc.SVD_CASES))
def test_svd_parity(name):
    c, mdl = device_svd(name)
    g = load_golden("svd_" + name)
    U, S, V = mdl.U, mdl.S, mdl.V
    assert U.dtype == S.dtype == V.dtype == np.float64
    rank = int(g["rank"])
    assert S.shape == (rank, rank) and U.shape == (c["data"].shape[0], rank) and V.shape == (rank, c["data"].shape[1])
    assert np.array_equal(S, np.diag(np.diag(S)))
    s_np = np.linalg.svd(c["data"].astype(np.float64), compute_uv=False)[:rank]
    ds = float(np.max(np.abs(np.diag(S) - s_np) / s_np))
    d = sc.svd_deviation(c["data"], (U, S, V), (c["U"], c["S"], c["V"]))
    lead = int(g["lead"])
    dg = sc.svd_deviation(c["data"], (U[:, :lead], S[:lead, :lead], V[:lead]), (g["U"], np.diag(g["S"][:lead]), g["V"]))
    E = V.T if c["left"] else U
    ortho = float(np.max(np.abs(np.dot(E.T, E) - np.eye(rank))))
    dfn = abs(mdl.frobenius_norm() - c["ferr"]) / np.linalg.norm(c["data"].astype(np.float64))
    print("%s rank %d  S vs numpy %.3e  U %.3e (golden %.3e, tol %.3e)  V %.3e (golden %.3e, tol %.3e)  ortho %.3e  "
          "frobenius_norm %.3e (tol %.3e)" % (name, rank, ds, d["U"], dg["U"], sc.device_tol("U"), d["V"], dg["V"], sc.device_tol("V"),
                                               ortho, dfn, sc.device_tol("svd_ferr")))
    assert measured(ds, name + " S") <= S_RTOL
    assert measured(d["U"], name + " U") <= sc.device_tol("U")
    assert measured(d["V"], name + " V") <= sc.device_tol("V")
    assert measured(dg["U"], name + " U golden") <= sc.device_tol("U")
    assert measured(dg["V"], name + " V golden") <= sc.device_tol("V")
    assert measured(ortho, name + " orthonormality") <= ORTHO_TOL
    assert measured(dfn, name + " frobenius_norm") <= sc.device_tol("svd_ferr")


@pytest.mark.parametrize("name", ["29x2100", "2100x130", "300x40_rank25"])
def test_svd_two_runs_same_bits(name):
    c, mdl = device_svd(name)
    again = pymf_amd.SVD(c["data"])
    again.factorize()
    assert np.array_equal(again.U, mdl.U) and np.array_equal(again.S, mdl.S) and np.array_equal(again.V, mdl.V)
    U, S, V = mdl.U, mdl.S, mdl.V
    mdl.factorize()                                            # the same object, the same context
    assert np.array_equal(mdl.U, U) and np.array_equal(mdl.S, S) and np.array_equal(mdl.V, V)


@pytest.mark.parametrize("name", sorted(sc.PCA_CASES))
def test_pca_parity(name):
    c = sc.pca_case(name)
    g = load_golden("pca_" + name)
    mdl = pymf_amd.PCA(c["data"], num_bases=c["num_bases"], center_mean=c["center_mean"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pymf_amd.nmf.PrecisionWarning)
        mdl.factorize(niter=5)
    assert mdl.ferr.shape == (1,)
    assert mdl.W.shape == g["W"].shape and mdl.H.shape == g["H"].shape and mdl.W.dtype == mdl.H.dtype == np.float64
    got = dict(W=mdl.W, H=mdl.H, eigenvalues=mdl.eigenvalues, ferr=mdl.ferr[0])
    want = dict(c["oracle"], W=g["W"], H=g["H"], eigenvalues=g["eigenvalues"], ferr=float(g["ferr"][0]))
    d = sc.pca_deviation(got, want)
    s_np = np.linalg.svd(so.f32(c["oracle"]["data"]), compute_uv=False)[:len(mdl.eigenvalues)]
    ds = float(np.max(np.abs(mdl.eigenvalues - s_np) / s_np))
    print("%s W %.3e (tol %.3e)  H %.3e (tol %.3e)  ferr %.3e (tol %.3e)  eigenvalues %.3e (tol %.3e; vs numpy on the float32 data %.3e)" % (
        name, d["W"], sc.device_tol("W"), d["H"], sc.device_tol("H"), d["ferr"], sc.device_tol("ferr"), d["eigenvalues"],
        sc.device_tol("eigenvalues"), ds))
    assert measured(d["W"], name + " W") <= sc.device_tol("W")
    assert measured(d["H"], name + " H") <= sc.device_tol("H")
    assert measured(d["ferr"], name + " ferr") <= sc.device_tol("ferr")
    assert measured(d["eigenvalues"], name + " eigenvalues") <= sc.device_tol("eigenvalues")
    assert measured(ds, name + " singular values") <= S_RTOL


def test_pca_user_w_docstring_example():
    g = load_golden("pca_doc_userw")
    mdl = pymf_amd.PCA(g["data"], num_bases=2)
    mdl.W = g["W"].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pymf_amd.nmf.PrecisionWarning)
        mdl.factorize(compute_w=False)
    assert np.array_equal(mdl.W, g["W"])
    assert mdl.H.shape == (2, 1) and np.array_equal(mdl.H, g["H"]) and mdl.ferr[0] == g["ferr"][0]
    # ... and without centring the coefficients are the data themselves
    raw = pymf_amd.PCA(g["data"].astype(np.float32), num_bases=2, center_mean=False)
    raw.W = g["W"].copy()
    raw.factorize(compute_w=False)
    assert np.array_equal(raw.H, g["data"].astype(np.float32).astype(np.float64))


def test_pca_hooks_by_hand_and_second_run_same_bits():
    c = sc.pca_case("29x300_k5")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pymf_amd.nmf.PrecisionWarning)
        ref = pymf_amd.PCA(c["data"], num_bases=5)
        ref.factorize()
        W, H, ferr = np.array(ref.W), np.array(ref.H), ref.ferr[0]
        ref.factorize()
        assert np.array_equal(ref.W, W) and np.array_equal(ref.H, H) and ref.ferr[0] == ferr
        mdl = pymf_amd.PCA(c["data"], num_bases=5)
        mdl.update_w()
        mdl.update_h()
    assert np.array_equal(mdl.W, W) and np.array_equal(mdl.H, H) and mdl.frobenius_norm() == ferr
    assert np.array_equal(mdl.eigenvalues, ref.eigenvalues) and mdl.eigenvalues.shape == (5,)


def test_cabi_alone():
    c = sc.svd_case("37x29")
    m, n = c["data"].shape
    ctx = _lib.Context(_lib.ALGO_PCA, m, n, min(m, n))
    with pytest.raises(_lib.PmfError):
        ctx.svd_rank()                                         # nothing decomposed yet
    ctx.set_v_dense(c["data"])
    rank = ctx.svd_decompose()
    assert rank == c["S"].shape[0] == ctx.svd_rank()
    U, S, V = ctx.svd_get(rank)
    assert sc.svd_deviation(c["data"], (U, np.diag(S), V), (c["U"], c["S"], c["V"]))["U"] <= sc.device_tol("U")
    assert ctx.svd_get(rank, want="S")[0] is None
    assert ctx.path_name == "svd_gram_f64"
    ctx.close()
