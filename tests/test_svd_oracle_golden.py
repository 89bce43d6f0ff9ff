"""The float64 oracle of SVD / PCA (tests/svd_oracle.py) equals the goldens that the real reference produced
(tests/golden/gen_golden_svd.py), up to the free sign of a singular pair and eigh's rounding (no GPU)."""
import numpy as np
import pytest

import svd_cases as sc
import svd_oracle as so
from conftest import load_golden

TOL = 1e-9      # eigh against eigh on the same float64 Gram matrix: rounding over the smallest relative gap (5 %)


@pytest.mark.parametrize("name", sorted(sc.SVD_CASES))
def test_svd_oracle_equals_reference(name):
    g, c = load_golden("svd_" + name), sc.svd_case(name)
    lead = int(g["lead"])
    assert c["S"].shape[0] == int(g["rank"])
    assert np.max(np.abs(np.diag(c["S"]) - g["S"]) / g["S"]) <= 1e-12
    Uo, Vo = so.fix_svd_signs(c["U"][:, :lead], c["V"][:lead], c["left"])
    Ug, Vg = so.fix_svd_signs(g["U"], g["V"], c["left"])
    assert sc.max_abs(Uo, Ug) <= TOL and sc.max_abs(Vo, Vg) <= TOL
    assert abs(c["ferr"] - float(g["ferr"])) <= 1e-9 * np.linalg.norm(c["data"])


@pytest.mark.parametrize("name", sorted(sc.PCA_CASES))
def test_pca_oracle_equals_reference(name):
    g, c = load_golden("pca_" + name), sc.pca_case(name)
    o = c["oracle"]
    assert o["W"].shape == g["W"].shape and o["H"].shape == g["H"].shape
    d = sc.pca_deviation(dict(W=g["W"], H=g["H"], eigenvalues=g["eigenvalues"], ferr=g["ferr"][0]), o)
    print(name, d)
    assert max(d.values()) <= TOL


def test_pca_user_w_golden():
    g = load_golden("pca_doc_userw")
    assert np.allclose(g["cdata"], 0.0)                        # one sample: centring leaves zeros (pca.py:79-80)
    assert np.array_equal(g["H"], np.zeros((2, 1))) and g["ferr"][0] == 0.0


def test_twin_rounds_only_what_the_device_rounds():
    c = sc.svd_case("29x300")
    U, S, V = so.svd(c["data"], f32_twin=True)
    assert np.array_equal(U, c["U"]) and np.array_equal(S, c["S"])          # float32-representable data: the eigen side is the oracle's
    assert np.array_equal(V, V.astype(np.float32).astype(np.float64)) and not np.array_equal(V, c["V"])
