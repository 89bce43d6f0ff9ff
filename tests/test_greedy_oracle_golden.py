"""tests/greedy_oracle.py against goldens of the real reference (tests/golden/gen_golden_greedy.py): selections exact."""
import os

import numpy as np
import pytest

import greedy_cases as gc
import greedy_oracle as go

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def test_doc_case():
    g = load("greedy_doc_2x3")
    r = go.factorize(g["data"], 2)
    assert r["select"] == g["select"].tolist()
    assert np.array_equal(r["W"], g["W"]) and np.allclose(r["H"], g["H"], rtol=0, atol=1e-12)
    assert g["ferr"].shape == (2,)                             # niter = 10: cut at i = 2 (nmf.py:198-202)
    assert np.allclose(g["ferr"], r["ferr"], rtol=0, atol=1e-12)


def test_doc_user_w():
    g = load("greedy_doc_userw")
    H = go.update_h(g["data"], g["W"])
    assert np.allclose(H, g["H"], rtol=0, atol=1e-12)
    assert abs(go.ferr(g["data"], g["W"], H) - float(g["ferr"])) <= 1e-12


@pytest.mark.parametrize("name", ["29x300_k6", "300x29_k6", "37x29_k5"])
def test_case(name):
    g = load("greedy_" + name)
    d = gc.data(name).astype(np.float64)
    r = go.factorize(d, len(g["select"]))
    assert r["select"] == g["select"].tolist()
    assert gc.rel_max(r["H"], g["H"]) <= 1e-9
    assert abs(r["ferr"] - float(g["ferr"])) <= 1e-9 * np.linalg.norm(d)


def test_niter3_golden_has_two_equal_entries():
    g = load("greedy_29x300_k6_niter3")
    assert g["ferr"].shape == (2,) and g["ferr"][0] == g["ferr"][1]
    assert g["select"].tolist() == gc.case("29x300_k6")["select"]


@pytest.mark.parametrize("name", ["40x300", "300x40"])
def test_greedycur(name):
    g = load("greedycur_" + name)
    c = gc.cur_case(name)
    assert c["rid"] == g["rid"].tolist() and c["cid"] == g["cid"].tolist()
    assert gc.rel_max(c["U"], g["U"]) <= 1e-9
    assert abs(c["ferr"] - float(g["ferr"])) <= 1e-9 * np.linalg.norm(c["data"].astype(np.float64))
