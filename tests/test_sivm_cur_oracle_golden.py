"""The oracle of tests/sivm_cur_cases.py against goldens of the real reference (tests/golden/gen_golden_sivm_cur.py):
selections exact."""
import os

import numpy as np
import pytest

import sivm_cur_cases as cc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", cc.GOLDEN)
def test_case(name):
    g = np.load(os.path.join(GOLD, "sivmcur_" + name + ".npz"))
    c = cc.case(name)
    assert str(g["case"]) == name and bool(g["cosine_patched"]) == (c["metric"] == "cosine")
    assert c["rid"] == g["rid"].tolist() and c["cid"] == g["cid"].tolist()
    assert cc.rel_max(c["U"], g["U"]) <= 1e-9
    assert abs(c["ferr"] - float(g["ferr"])) <= 1e-9 * np.linalg.norm(c["data"].astype(np.float64))


def test_doc_case_holds_the_docstring_data():
    g = np.load(os.path.join(GOLD, "sivmcur_doc_2x3.npz"))
    assert np.array_equal(g["data"], np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]]))    # sivm_cur.py:55
    assert g["rid"].tolist() == [-1] and g["cid"].tolist() == [-1]
