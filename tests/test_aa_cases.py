"""The AA cases leave float32 room (no GPU): H0 has full row rank with a margin, the restated device rounds stay within half
the round cap and inside the corral bound, and forming W_hat from a float32 product and rounding V, R, X and g to float32 moves the oracle's W, H and ferr by no
more than the figures that the device tolerances are derived from (tests/aa_cases.py)."""
import os
import re

import numpy as np
import pytest

import aa_cases as ac
import aa_oracle as ao
import sivm_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_match_the_library():
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_host_aa.h")) as f:
        host = f.read()
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_aa.h")) as f:
        dev = f.read()
    assert int(re.search(r"PMF_AA_ROUND_CAP = (\d+);", host).group(1)) == ac.ROUND_CAP
    assert float(re.search(r"PMF_AA_TAU = ([0-9.e-]+);", host).group(1)) == ao.AA_TAU
    assert float(re.search(r"PMF_AA_RHO = ([0-9.e-]+);", host).group(1)) == ao.AA_RHO
    assert float(re.search(r"PMF_AA_PIV = ([0-9.e-]+);", host).group(1)) == ao.AA_PIV
    assert int(re.search(r"PMF_AA_MAX_CORRAL = (\d+);", dev).group(1)) == ac.MAX_CORRAL


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_case_leaves_float32_room(name):
    c = ac.case(name)
    V64 = c["V"].astype(np.float64)
    s = np.linalg.svd(c["H0"], compute_uv=False)
    assert s[-1] / s[0] >= ac.MIN_RANK_MARGIN
    assert min(V64.shape[0] + 1, V64.shape[1]) <= ac.MAX_CORRAL
    W64, b64, r64, corral64 = ao.device_rounds(V64, c["Wh"])
    Wh32 = ao.w_hat_f32(V64, c["H0"])
    Wf, bf, r32, corral32 = ao.device_rounds(V64, Wh32, f32_v=True, f32_r=True, f32_g=True)
    dw64 = np.linalg.norm(W64 - c["W"]) / np.linalg.norm(c["W"])
    dw = np.linalg.norm(Wf - c["W"]) / np.linalg.norm(c["W"])
    Hf, ferr_f = so.update_h(V64, Wf, f32_v=True, f32_w=True, f32_rhs=True, f32_x=True)
    dh = np.linalg.norm(Hf - c["H"]) / np.linalg.norm(c["H"])
    df = abs(ferr_f - c["ferr"]) / c["ferr"]
    print("%s rounds %d / %d corral %d / %d  W %.3e (float64 rounds %.3e)  H %.3e  ferr %.3e" % (name, r64, r32, corral64, corral32, dw, dw64, dh, df))
    assert max(r64, r32) <= ac.ROUND_CAP // 2
    assert dw <= ac.MEASURED_W and dw64 <= ac.MEASURED_W
    assert dh <= ac.MEASURED_H
    assert df <= ac.MEASURED_FERR
    for i in range(c["k"]):                                    # the certificate holds for the float32 rounds' weights
        assert ao.gap(V64, Wh32[:, i], bf[i]) <= 2.0 * ao.AA_TAU * (np.abs(V64).max() ** 2) * V64.shape[0]
    assert bf.min() >= 0.0 and np.abs(bf.sum(axis=1) - 1.0).max() <= 1e-12


def test_inside_case_returns_w_hat():
    c = ac.case("12x200_k4_inside")
    assert np.linalg.norm(c["W"] - c["Wh"]) <= 1e-12 * np.linalg.norm(c["Wh"])
    assert max(ao.gap(c["V"].astype(np.float64), c["Wh"][:, i], c["beta"][i]) for i in range(c["k"])) <= 1e-12


def test_duplicate_columns_lowest_index_and_no_twin():
    c = ac.case("16x200_k4_dup")
    V = c["V"]
    assert np.array_equal(V[:, 5], V[:, 150]) and np.array_equal(V[:, 6], V[:, 150]) and np.array_equal(V[:, 90], V[:, 17])
    for b in c["beta"]:
        assert b[6] == 0.0 and b[150] == 0.0 and b[90] == 0.0          # only the lowest index of a set of twins is ever taken
    # a corral that is offered the twin of one of its columns refuses it: the pivot of the entering column is zero
    w = c["Wh"][:, 0]
    G = (V[:, [5, 17, 150]].astype(np.float64) - w[:, None])
    A = G.T.dot(G)
    try:
        p = ao._affine_min(A, [0, 1, 2])[1]
    except np.linalg.LinAlgError:
        p = 0.0
    assert not (p > ao.AA_PIV * (A[-1, -1] + 1.0))
    assert ao._affine_min(A, [0, 1])[1] > ao.AA_PIV * (A[1, 1] + 1.0)          # (the two distinct columns are admitted)


def test_hull_qp_small_known_answers():
    V = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.allclose(V.dot(ao.hull_qp(V, np.array([0.25, 0.25]))), [0.25, 0.25])         # inside
    assert np.allclose(V.dot(ao.hull_qp(V, np.array([1.0, 1.0]))), [0.5, 0.5])             # onto an edge
    assert np.allclose(ao.hull_qp(V, np.array([-1.0, -2.0])), [1.0, 0.0, 0.0])             # onto a vertex
    rng = np.random.RandomState(0)
    V = rng.randn(5, 12)                                                                   # n > m: the Hessian of the posed QP is singular
    w = 3.0 * rng.randn(5)
    b = ao.hull_qp(V, w)
    assert b.min() >= 0 and abs(b.sum() - 1) < 1e-12 and ao.gap(V, w, b) <= 1e-12
