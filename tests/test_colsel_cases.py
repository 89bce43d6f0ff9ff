"""The conditions under which the device comparison of tests/test_gpu_colsel.py means something, on the float64 oracle alone
(no GPU): a clear argmax at every selection step, in float64 and with the fp32-formed quantities rounded through float32, the
same selections either way, a well-conditioned W^T W, the reference goldens, and the float32 deviations of H and ferr that the
device tolerances are made of."""
import functools

import numpy as np
import pytest

import colsel_cases as cc
import sivm_cases as sc
import sivm_oracle as so
from conftest import load_golden

NAMES = sorted(cc.CASES)
SELECT_NAMES = NAMES + sorted(cc.PANEL_CASES)       # the panel cases compare selection and W only
GOLDENS = ["laesa_doc_2x3_k2", "laesa_doc_userw", "laesa_29x300_k6_l2", "laesa_29x300_k6_l1", "laesa_29x300_k6_cosine",
           "laesa_29x300_k6_origin", "gmap_doc_2x3_k2", "gmap_doc_userw", "gmap_29x300_k6_pca", "gmap_29x300_k6_aa",
           "gmap_29x300_k6_nmf", "gmap_37x29_k5"]


@functools.lru_cache(maxsize=None)
def f32_run(name):
    """(select, scores) of the oracle with the device's fp32 quantities rounded through float32"""
    scores = []
    select, _ = cc.oracle(name, cc.case(name)["V"].astype(np.float64), f32_ops=True, scores=scores)
    return select, scores


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_argmax_gap(name):
    c = cc.case(name)
    for label, scores in (("float64", c["scores"]), ("float32 operands", f32_run(name)[1])):
        assert len(scores) == (c["k"] if c["rule"] == "gmap" or c["init"] == "fastmap" else c["k"] - 1)
        for step, gap in enumerate(cc.gaps(scores, c["special"])):
            assert gap >= cc.MIN_GAP, "%s %s step %d: gap %.2e" % (name, label, step, gap)


@pytest.mark.parametrize("name", ["laesa_16x640_k4_tie", "gmap_16x640_k4_tie"])
def test_the_tie_is_a_tie(name):
    c = cc.case(name)
    twin = [j for j in range(cc.TIE_COLUMN) if np.array_equal(c["V"][:, j], c["V"][:, cc.TIE_COLUMN])]
    assert len(twin) == 1
    assert twin[0] in c["select"] and cc.TIE_COLUMN not in c["select"]          # the lowest index wins
    assert any(np.sort(s)[-1] == np.sort(s)[-2] for s in c["scores"])           # ... a tie on top of an argmax


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_selection_is_stable_under_fp32_and_reaches_its_range(name):
    c = cc.case(name)
    assert f32_run(name)[0] == c["select"]
    assert len(set(c["select"])) == c["k"]
    n = c["V"].shape[1]
    if c["rule"] == "laesa" and c["init"] == "fastmap":
        assert sorted(c["select"]) == sorted(c["verts"])
    if c["special"] in ("ends", "trip2"):   # winners in the first and in the last workgroup
        assert min(c["select"]) < 64 and max(c["select"]) >= n - 64
    if c["special"] == "trip2":             # a winner that only the second trip of the quad loop sees
        assert cc.TRIP2_COLUMN in c["select"]
    if name in cc.PANEL_CASES:              # the shapes whose panel ranges tests/test_sivm_cases.py restates
        assert (c["V"].shape[0], n) in {(s[0], s[1]) for s in sc.PANEL_CASES.values()}
    else:
        assert -(-n // 64) <= 1024          # one panel per workgroup


def test_the_shapes_cover_every_row_tail():
    tails = {cc.spec(n)[0]: set() for n in NAMES}
    for n in NAMES:
        tails[cc.spec(n)[0]].add(cc.spec(n)[1] % 4)
    assert tails == {"laesa": {0, 1, 2, 3}, "gmap": {0, 1, 2, 3}}
    assert {cc.spec(n)[5] for n in NAMES if cc.spec(n)[0] == "laesa"} == {"l2", "l1", "cosine"}
    assert {cc.spec(n)[5] for n in NAMES if cc.spec(n)[0] == "gmap"} == {"pca", "aa", "nmf"}
    assert cc.case("gmap_29x300_k6_nmf")["V"].min() == 0.0                      # shifted non-negative


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_condition_number(name):
    W = cc.case(name)["W"]
    assert np.linalg.cond(W.T.dot(W)) <= cc.MAX_COND


def golden_v(g):
    if "case" in g:
        rule, m, n, k, seed, what, _, special = cc.CASES[str(g["case"])]
        return cc.data(rule, m, n, k, seed, what, special)[0]
    return g["V"]


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_reproduces_golden(name):
    """select and W exactly, H and ferr to the float64 tolerances of tests/test_sivm_oracle_golden.py"""
    g = load_golden(name)
    V = golden_v(g).astype(np.float64)
    if "select" in g:
        if name.startswith("laesa"):
            select, W = cc.co.laesa_update_w(V, int(g["k"]), str(g["metric"]), str(g["init"]))
        else:
            select, W = cc.co.gmap_update_w(V, int(g["k"]), str(g["method"]))
        assert select == [int(s) for s in g["select"]]
        assert np.array_equal(W, g["W"])
        if "case" in g:
            assert select == cc.case(str(g["case"]))["select"]
    H, ferr = so.update_h(V, g["W"])
    assert np.abs(H - g["H"]).max() <= 1e-10
    assert abs(ferr - g["ferr"][0]) <= 1e-10 * max(1.0, g["ferr"][0])
    if name == "laesa_29x300_k6_cosine":
        assert bool(g["cosine_patched"])


def test_origin_uses_the_last_column():
    g = load_golden("laesa_29x300_k6_origin")
    assert int(g["select"][0]) == -1
    assert np.array_equal(g["W"][:, 0], golden_v(g)[:, -1].astype(np.float64))


@functools.lru_cache(maxsize=None)
def deviation(name):
    """(H relative Frobenius, ferr relative): the all-float64 oracle against float32 V, W, right-hand sides and X"""
    c = cc.case(name)
    H32, ferr32 = so.update_h(c["V"].astype(np.float64), c["W"], True, True, True, True)
    return np.linalg.norm(H32 - c["H"]) / np.linalg.norm(c["H"]), abs(ferr32 - c["ferr"]) / c["ferr"]


@pytest.mark.parametrize("name", NAMES)
def test_fp32_deviation(name):
    dh, df = deviation(name)
    print("%s: H deviation %.3e, ferr deviation %.3e" % (name, dh, df))
    assert dh <= cc.MEASURED_H * 1.001 and df <= cc.MEASURED_FERR * 1.001      # the figures H_TOL / FERR_TOL are made of


def test_the_measured_figures_are_attained():
    """MEASURED_H / MEASURED_FERR are the worst over the cases, not a bound above it."""
    dev = [deviation(name) for name in NAMES]
    assert max(d[0] for d in dev) >= cc.MEASURED_H * 0.999 and max(d[1] for d in dev) >= cc.MEASURED_FERR * 0.999
