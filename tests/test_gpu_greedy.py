"""pymf_amd.GREEDY / GREEDYCUR on the device against the float64 oracle (tests/greedy_oracle.py) on the cases of
tests/greedy_cases.py, and against goldens of the real reference.

The rank case (29 x 300 of rank 3, 5 bases): the first two selections are the oracle's; the third round is an exact tie in
exact arithmetic (greedy_cases.py), so the third selection must be one of the tied columns; all five are valid indices."""
import os

import numpy as np
import pytest

import greedy_cases as gc
import greedy_oracle as go

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pm():
    import pymf_amd
    return pymf_amd


def run(pm, name, **kw):
    c = gc.case(name)
    np.random.seed(3)
    mdl = pm.GREEDY(c["data"], num_bases=c["num_bases"])
    mdl.factorize(**kw)
    return c, mdl


@pytest.mark.parametrize("name", gc.h_cases())
def test_case_matches_the_oracle(pm, name):
    c, mdl = run(pm, name)
    print(name, mdl.select, "H", gc.rel_max(mdl.H, c["H"]), "ferr", abs(mdl.ferr[0] - c["ferr"]) / np.linalg.norm(c["data"].astype(np.float64)))
    assert mdl.select == c["select"] and all(type(s) is int for s in mdl.select)
    assert mdl.W.dtype == np.float32 and np.array_equal(mdl.W, c["data"][:, c["select"]])
    assert mdl.H.dtype == np.float64 and mdl.H.shape == c["H"].shape
    assert gc.rel_max(mdl.H, c["H"]) <= gc.device_tol_h()
    assert mdl.ferr.shape == (1,)
    assert abs(mdl.ferr[0] - c["ferr"]) <= gc.device_tol_ferr() * np.linalg.norm(c["data"].astype(np.float64))


@pytest.mark.parametrize("name", list(gc.SELECT_CASES))
def test_selection_of_the_wide_and_panel_cases(pm, name):
    """Eight operand tiles on every wave, more than one panel per workgroup, a second trip of the panel loop with one and with two
    row chunks, and more candidates in Gram space than k_greedy_gram has threads (greedy_cases.SELECT_CASES)."""
    c, mdl = run(pm, name, compute_h=False, compute_err=False)
    print(name, mdl.select[:8], c["select"][:8], min(c["gaps"]))
    assert mdl.select == c["select"] and all(type(s) is int for s in mdl.select)
    assert mdl.W.dtype == np.float32 and np.array_equal(mdl.W, c["data"][:, c["select"]])


def test_planted_tie_takes_the_lower_index(pm):
    c, mdl = run(pm, gc.TIE_CASE, compute_h=False, compute_err=False)
    src, dup = gc.tie_columns(gc.spectrum_data(64, 640, 8))
    assert mdl.select[0] == src and dup not in mdl.select and mdl.select == c["select"]


def test_rank_deficient_data(pm):
    c, mdl = run(pm, gc.RANK_CASE, compute_h=False, compute_err=False)
    print(mdl.select, c["select"])
    assert mdl.select[:gc.RANK - 1] == c["select"][:gc.RANK - 1]
    T = c["scores"][gc.RANK - 1]
    assert T[mdl.select[gc.RANK - 1]] >= T.max() * (1.0 - gc.TIE_RTOL)
    assert len(mdl.select) == 5 and all(0 <= s < 300 for s in mdl.select)
    assert np.array_equal(mdl.W, c["data"][:, mdl.select])


def test_compute_h_false_leaves_no_h_result(pm):
    c = gc.case("29x300_k6")
    np.random.seed(5)
    mdl = pm.GREEDY(c["data"], num_bases=6)
    mdl.factorize(compute_h=False, compute_err=False)
    assert mdl.select == c["select"] and not hasattr(mdl, "ferr")
    np.random.seed(5)
    np.random.random((29, 6))                                     # NMF.init_w's draw
    assert np.array_equal(mdl.H, np.random.random((6, 300)))      # NMF.init_h's draw, untouched


def test_user_w_matches_the_golden(pm):
    g = np.load(os.path.join(GOLD, "greedy_doc_userw.npz"))
    mdl = pm.GREEDY(g["data"], num_bases=2)
    mdl.W = g["W"].copy()
    mdl.factorize(compute_w=False)
    assert mdl.H.dtype == np.float64 and gc.rel_max(mdl.H, g["H"]) <= gc.device_tol_h()
    assert np.array_equal(mdl.W, g["W"])
    assert abs(mdl.ferr[0] - float(g["ferr"])) <= gc.device_tol_ferr() * np.linalg.norm(g["data"])


def test_doc_case_against_the_golden(pm):
    """greedy.py:57-59.  The data have rank 2 and two bases are asked for: behind the first selection (column 2) the residuals
    of columns 0 and 1 lie on one line and their scores are equal in exact arithmetic (both |B'|^2), so the second selection
    is either of them -- the reference's rounding takes column 0 -- and the fit is exact with both."""
    g = np.load(os.path.join(GOLD, "greedy_doc_2x3.npz"))
    assert g["select"].tolist() == [2, 0]
    mdl = pm.GREEDY(g["data"], num_bases=2)
    mdl.factorize()
    assert mdl.select[0] == 2 and mdl.select[1] in (0, 1)
    assert mdl.W.dtype == np.float64 and np.array_equal(mdl.W, g["data"][:, mdl.select])
    assert mdl.H.dtype == np.float64 and gc.rel_max(mdl.H, go.update_h(g["data"], mdl.W)) <= gc.device_tol_h()
    assert abs(mdl.ferr[0] - g["ferr"][0]) <= gc.device_tol_ferr() * np.linalg.norm(g["data"])


def test_hooks_by_hand_and_second_run(pm):
    c, mdl = run(pm, "130x1000_k12")
    W1, H1, f1, s1 = mdl.W.copy(), mdl.H.copy(), mdl.ferr.copy(), list(mdl.select)
    mdl.factorize()
    assert mdl.select == s1 and np.array_equal(mdl.W, W1) and np.array_equal(mdl.H, H1) and np.array_equal(mdl.ferr, f1)
    hand = pm.GREEDY(c["data"], num_bases=c["num_bases"])
    hand.update_w()
    hand.update_h()
    assert hand.select == s1 and np.array_equal(hand.W, W1) and np.array_equal(hand.H, H1)
    assert hand.frobenius_norm() == f1[0]


def test_data_replaced_in_place_is_noticed(pm):
    c = gc.case("29x300_k6")
    d = c["data"].copy()
    mdl = pm.GREEDY(d, num_bases=6)
    mdl.factorize(compute_err=False)
    assert mdl.select == c["select"]
    d[:] = gc.REPLACED_DATA()
    gaps = []
    want = go.select(d.astype(np.float64), 6, gaps=gaps)
    assert min(gaps) >= gc.MIN_GAP and want != c["select"]
    mdl.factorize(compute_h=False, compute_err=False)
    assert mdl.select == want and np.array_equal(mdl.W, d[:, want])


def test_niter3_cuts_ferr_to_two_entries(pm):
    g = np.load(os.path.join(GOLD, "greedy_29x300_k6_niter3.npz"))
    c = gc.case("29x300_k6")
    mdl = pm.GREEDY(c["data"], num_bases=6)
    mdl.factorize(niter=3)
    assert mdl.ferr.shape == (2,) and g["ferr"].shape == (2,)
    assert np.all(np.abs(mdl.ferr - g["ferr"]) <= gc.device_tol_ferr() * np.linalg.norm(c["data"].astype(np.float64)))
    assert mdl.select == [int(s) for s in g["select"]]


def test_cabi_alone(pm):
    from pymf_amd import _lib
    c = gc.case("29x300_k6")
    ctx = _lib.Context(_lib.ALGO_GREEDY, 29, 300, 6)
    try:
        ctx.set_v_dense(c["data"])
        ctx.update_w()
        assert ctx.get_select().tolist() == c["select"]
        assert np.array_equal(ctx.get_w(), c["data"][:, c["select"]])
        ctx.update_h()
        assert gc.rel_max(ctx.get_h64(), c["H"]) <= gc.device_tol_h()
        assert abs(ctx.frobenius() - c["ferr"]) <= gc.device_tol_ferr() * np.linalg.norm(c["data"].astype(np.float64))
        assert ctx.greedy_select(6).tolist() == c["select"]
    finally:
        ctx.close()


def test_cabi_widest_operand_twice(pm):
    """pmf_greedy_select with 64 bases (k_greedy_pass<4> .. <8>): the oracle's list, and the same list from a second call."""
    from pymf_amd import _lib
    c = gc.case("80x640_k64")
    ctx = _lib.Context(_lib.ALGO_GREEDY, 80, 640, 64)
    try:
        ctx.set_v_dense(c["data"])
        first = ctx.greedy_select(64)
        assert first.dtype == np.int32 and first.tolist() == c["select"]
        assert np.array_equal(ctx.greedy_select(64), first)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(gc.GREEDYCUR_CASES))
def test_greedycur(pm, name):
    c = gc.cur_case(name)
    mdl = pm.GREEDYCUR(c["data"], rrank=c["rrank"])
    mdl.factorize()
    nrm = np.linalg.norm(c["data"].astype(np.float64))
    print(name, gc.rel_max(mdl.S, c["U"]), c["tol_U"], abs(mdl.frobenius_norm() - c["ferr"]) / nrm)
    assert list(mdl._rid) == c["rid"] and list(mdl._cid) == c["cid"]
    assert np.array_equal(mdl.U, c["data"][:, c["cid"]].astype(np.float64))
    assert np.array_equal(mdl.V, c["data"][c["rid"], :].astype(np.float64))
    assert gc.rel_max(mdl.S, c["U"]) <= c["tol_U"]
    assert abs(mdl.frobenius_norm() - c["ferr"]) <= gc.device_tol_ferr() * nrm
    assert mdl.sample(mdl.data, c["rrank"]) == c["cid"]


def test_limits(pm):
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(ValueError):
        pm.GREEDY(np.ones((8, 100), dtype=np.float32), num_bases=65).factorize()
    with pytest.raises(TypeError):
        pm.GREEDY(sp.csr_matrix(np.ones((3, 5))), num_bases=2).factorize()
    with pytest.raises(ValueError):
        pm.GREEDY(np.ones((2433, 2433), dtype=np.float32), num_bases=2).factorize()
    with pytest.raises(ValueError):
        pm.GREEDYCUR(np.ones((80, 100), dtype=np.float32), rrank=65).factorize()
