"""pymf_amd.SIVM on the MI355X against the float64 oracle (tests/sivm_oracle.py) on the cases of tests/sivm_cases.py and the
reference goldens.  select and W must be exact; H and ferr within the tolerances that sivm_cases derives from the oracle's
own float32 error (4 x the measured worst)."""
import ctypes

import numpy as np
import pytest

import pymf_amd
import sivm_cases as sc
from conftest import close, load_golden, rel_fro
from pymf_amd import _lib

pytestmark = pytest.mark.gpu


def device(name, **kw):
    c = sc.case(name)
    mdl = pymf_amd.SIVM(c["V"], num_bases=c["k"], dist_measure=c["metric"], init=c["init"])
    mdl.factorize(**kw)
    return c, mdl


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_parity(name):
    c, mdl = device(name)
    print("%s select %s" % (name, mdl.select))
    assert mdl.select == c["select"]
    assert all(type(s) is int for s in mdl.select)
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), c["V"][:, c["select"]])
    H = np.asarray(mdl.H)
    assert H.dtype == np.float64 and H.shape == c["H"].shape
    dh = rel_fro(H, c["H"], name + " H")
    df = abs(mdl.ferr[0] - c["ferr"]) / c["ferr"]
    print("%s H deviation %.3e (tol %.3e)  ferr deviation %.3e (tol %.3e)  min H %.3e  max |sum - 1| %.3e" % (
        name, float(dh), sc.H_TOL, df, sc.FERR_TOL, H.min(), np.abs(H.sum(axis=0) - 1.0).max()))
    assert dh <= sc.H_TOL
    close(mdl.ferr[0], c["ferr"], rtol=sc.FERR_TOL, what=name + " ferr")
    assert H.min() >= 0.0
    assert np.abs(H.sum(axis=0) - 1.0).max() <= 1e-5


@pytest.mark.parametrize("name", sorted(sc.PANEL_CASES))
def test_panel_ranges_select_and_w(name):
    """Several panels per workgroup in k_sivm_pass, every metric and the origin start: selection and W only (sivm_cases.py)."""
    c, mdl = device(name, compute_h=False, compute_err=False)
    print("%s select %s" % (name, mdl.select))
    assert mdl.select == c["select"]
    assert all(type(s) is int for s in mdl.select)
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), c["V"][:, c["select"]])


def test_panel_ranges_through_sivm_select():
    """The same ranges from SIVM_CUR's entry point, the column-panel pass forced: among the columns of the 8 x 65 600 data, and
    among the rows of a 65 600 x 8 copy (the pass then runs on a transposed copy made on the device)."""
    c = sc.case("8x65600_k3_l2")
    V = c["V"]
    for data, transposed in ((V, False), (np.ascontiguousarray(V.T), True)):
        ctx = _lib.Context(_lib.ALGO_CUR, data.shape[0], data.shape[1], c["k"])
        try:
            ctx.set_v_dense(data)
            got = ctx.sivm_select(c["k"], transposed, 0, 0, path=1)
            print(transposed, got.tolist())
            assert got.tolist() == c["select"]
        finally:
            ctx.close()


def test_compute_h_false_leaves_zeros():
    c, mdl = device("29x300_k6_l2", compute_h=False)
    assert mdl.select == c["select"]
    assert np.array_equal(mdl.H, np.zeros((c["k"], c["V"].shape[1])))


def test_user_w_matches_golden():
    g = load_golden("sivm_doc_userw")
    mdl = pymf_amd.SIVM(g["V"], num_bases=2)
    mdl.W = g["W"].copy()
    mdl.factorize(compute_w=False)
    assert np.array_equal(mdl.W, g["W"])
    close(mdl.H, g["H"], rtol=0, atol=1e-6, what="doc userw H")
    assert abs(mdl.ferr[0] - g["ferr"][0]) <= 1e-6


def test_hooks_by_hand_equal_factorize():
    c, ref = device("29x300_k6_l2")
    mdl = pymf_amd.SIVM(c["V"], num_bases=c["k"])
    mdl.update_w()
    mdl.update_h()
    assert mdl.select == ref.select
    assert np.array_equal(mdl.W, ref.W)
    assert np.array_equal(mdl.H, ref.H)
    assert mdl.frobenius_norm() == ref.ferr[0]


def test_second_factorize_same_bits():
    c, mdl = device("64x4113_k8")
    sel, W, H, ferr = list(mdl.select), np.array(mdl.W), np.array(mdl.H), mdl.ferr[0]
    mdl.factorize()
    assert mdl.select == sel
    assert np.array_equal(mdl.W, W) and np.array_equal(mdl.H, H) and mdl.ferr[0] == ferr


def test_data_replaced_in_place_is_noticed():
    c = sc.case("29x300_k6_l2")
    other = sc.case("29x300_k6_l1")
    V = np.array(c["V"])
    mdl = pymf_amd.SIVM(V, num_bases=c["k"])
    mdl.factorize()
    assert mdl.select == c["select"]
    V[:, :] = other["V"]
    mdl.factorize()
    assert mdl.select == sc.so.update_w(other["V"].astype(np.float64), other["k"])[0]


def test_cabi_alone():
    c = sc.case("5x37_k3")
    m, n = c["V"].shape
    ctx = _lib.Context(_lib.ALGO_SIVM, m, n, c["k"])
    ctx.set_v_dense(c["V"])
    ctx.update_w()
    assert [int(s) for s in ctx.get_select()] == c["select"]
    assert np.array_equal(ctx.get_w(), c["V"][:, c["select"]])
    ctx.close()


def test_singular_w_is_an_error():
    c = sc.case("29x300_k6_l2")
    mdl = pymf_amd.SIVM(c["V"], num_bases=3)
    W = np.array(c["V"][:, [5, 9, 5]], dtype=np.float64)         # a repeated column: W^T W is singular
    mdl.W = W
    with pytest.raises(_lib.PmfError, match="not unique"):
        mdl.factorize(compute_w=False)
