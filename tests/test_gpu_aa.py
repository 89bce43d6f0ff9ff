"""pymf_amd.AA on the MI355X against the float64 oracle (tests/aa_oracle.py) on the cases of tests/aa_cases.py, started from the
same W and H.  W, H and ferr within the tolerances that aa_cases derives from the oracle's own float32 error (4 x the
measured worst); beta is held to its constraints, to W = data beta^T and to the duality gap of its columns' problems."""
import numpy as np
import pytest

import pymf_amd
import aa_cases as ac
import aa_oracle as ao
from conftest import close, rel_fro
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

_runs = {}


def device(name):
    """One factorize() of the case through the class, kept for the tests that only read it."""
    if name not in _runs:
        c = ac.case(name)
        mdl = pymf_amd.AA(c["V"], num_bases=c["k"])
        mdl.W, mdl.H = c["W0"].copy(), c["H0"].copy()
        mdl.factorize(niter=1)
        _runs[name] = mdl
    return ac.case(name), _runs[name]


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_parity(name):
    c, mdl = device(name)
    W, H, beta = np.asarray(mdl.W), np.asarray(mdl.H), np.asarray(mdl.beta)
    V64 = c["V"].astype(np.float64)
    assert W.dtype == c["V"].dtype and W.shape == c["W"].shape
    assert H.dtype == np.float64 and H.shape == c["H"].shape
    assert beta.dtype == np.float64 and beta.shape == (c["k"], V64.shape[1])
    dw = rel_fro(W, c["W"], name + " W")
    dh = rel_fro(H, c["H"], name + " H")
    df = abs(mdl.ferr[0] - c["ferr"]) / c["ferr"]
    rounds = mdl._ctx.aa_rounds()
    gaps = [ao.gap(V64, c["Wh"][:, i], beta[i]) for i in range(c["k"])]
    bound = 2.0 * ao.AA_TAU * (np.abs(V64).max() ** 2) * V64.shape[0]
    print("%s rounds %d  W %.3e (tol %.3e)  H %.3e (tol %.3e)  ferr %.3e (tol %.3e)  min beta %.3e  max |sum - 1| %.3e  max gap %.3e (bound %.3e)" % (
        name, rounds, float(dw), ac.W_TOL, float(dh), ac.H_TOL, df, ac.FERR_TOL, beta.min(), np.abs(beta.sum(axis=1) - 1.0).max(), max(gaps), bound))
    assert dw <= ac.W_TOL
    assert dh <= ac.H_TOL
    close(mdl.ferr[0], c["ferr"], rtol=ac.FERR_TOL, what=name + " ferr")
    assert beta.min() >= 0.0
    assert np.abs(beta.sum(axis=1) - 1.0).max() <= 1e-6
    assert rel_fro(W, V64.dot(beta.T), name + " W = data beta^T") <= 2e-7          # W is the float32 rounding of data beta^T
    assert max(gaps) <= bound
    assert H.min() >= 0.0 and np.abs(H.sum(axis=0) - 1.0).max() <= 1e-5
    assert rounds <= ac.ROUND_CAP // 2
    if c["special"] == "dup":
        assert not beta[:, [6, 90, 150]].any()
    if c["special"] == "inside":
        assert rel_fro(W, c["Wh"], name + " W = W_hat") <= ac.W_TOL


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_hooks_by_hand_equal_factorize_and_second_run_same_bits(name):
    c, ref = device(name)
    mdl = pymf_amd.AA(c["V"], num_bases=c["k"])
    mdl.W, mdl.H = c["W0"].copy(), c["H0"].copy()
    mdl.update_w()
    beta = np.array(mdl.beta)
    mdl.update_h()
    assert np.array_equal(mdl.W, ref.W) and np.array_equal(mdl.H, ref.H) and np.array_equal(beta, ref.beta)
    assert mdl.frobenius_norm() == ref.ferr[0]
    again = pymf_amd.AA(c["V"], num_bases=c["k"])
    again.W, again.H = c["W0"].copy(), c["H0"].copy()
    again.factorize(niter=1)
    assert np.array_equal(again.W, ref.W) and np.array_equal(again.H, ref.H) and np.array_equal(again.beta, ref.beta)
    assert again.ferr[0] == ref.ferr[0]


def test_user_w_docstring_case():
    data = np.array([[1.5], [1.2]])                            # aa.py:72-76
    mdl = pymf_amd.AA(data, num_bases=2)
    mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    mdl.factorize(niter=5, compute_w=False)
    assert np.array_equal(mdl.W, np.array([[1.0, 0.0], [0.0, 1.0]]))
    H, ferr = ao.update_h(data, mdl.W)                         # the point of the simplex nearest (1.5, 1.2): (0.65, 0.35)
    close(mdl.H, H, rtol=0, atol=1e-6, what="doc userw H")
    assert np.allclose(H[:, 0], [0.65, 0.35])
    assert abs(mdl.ferr[0] - ferr) <= 1e-6


def test_three_iterations_ferr_does_not_increase():
    c = ac.case("29x300_k6")
    mdl = pymf_amd.AA(c["V"], num_bases=c["k"])
    mdl.W, mdl.H = c["W0"].copy(), c["H0"].copy()
    mdl.factorize(niter=3)
    assert len(mdl.ferr) == 3
    print("ferr", mdl.ferr)
    close(mdl.ferr[0], c["ferr"], rtol=ac.FERR_TOL, what="niter 3 first ferr")
    for i in (1, 2):                                           # both half steps minimise: the error cannot grow beyond rounding
        assert mdl.ferr[i] <= mdl.ferr[i - 1] * (1.0 + ac.FERR_TOL)
    V64 = c["V"].astype(np.float64)
    assert rel_fro(mdl.W, V64.dot(mdl.beta.T), "niter 3 W = data beta^T") <= 2e-7
    assert abs(np.linalg.norm(V64 - np.asarray(mdl.W, dtype=np.float64).dot(mdl.H)) - mdl.ferr[2]) <= 1e-5 * mdl.ferr[2]


def test_docstring_example_runs():
    data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])       # aa.py:58-66
    np.random.seed(7)
    mdl = pymf_amd.AA(data, num_bases=2)
    mdl.factorize(niter=5)
    assert mdl.W.shape == (2, 2) and mdl.H.shape == (2, 3) and mdl.beta.shape == (2, 3)
    assert mdl.beta.min() >= 0 and np.abs(mdl.beta.sum(axis=1) - 1).max() <= 1e-6
    assert np.all(np.diff(mdl.ferr) <= 1e-6)


def test_rank_deficient_h_is_an_error():
    c = ac.case("29x300_k6")
    mdl = pymf_amd.AA(c["V"], num_bases=c["k"])
    H = c["H0"].copy()
    H[3] = H[1]                                                # a repeated row: H H^T is singular
    mdl.W, mdl.H = c["W0"].copy(), H
    with pytest.raises(_lib.PmfError, match="rank deficient") as e:
        mdl.update_w()
    assert e.value.code == _lib.PMF_EINVAL


def test_cabi_alone():
    c = ac.case("37x29_k5")
    m, n = c["V"].shape
    ctx = _lib.Context(_lib.ALGO_AA, m, n, c["k"])
    assert ctx.path_name == "aa_pricing"
    ctx.set_v_dense(c["V"])
    ctx.set_h(c["H0"])
    with pytest.raises(_lib.PmfError, match="no beta yet"):
        ctx.get_beta()
    ctx.update_w()
    assert rel_fro(ctx.get_w(), c["W"], "cabi W") <= ac.W_TOL
    assert rel_fro(ctx.get_beta(), c["beta"], "cabi beta (n <= m: unique)") <= 10 * ac.W_TOL
    ctx.close()
    with pytest.raises(_lib.PmfError, match="corral bound"):
        _lib.Context(_lib.ALGO_AA, 200, 300, 4)
