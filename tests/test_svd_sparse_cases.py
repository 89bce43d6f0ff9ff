"""The sparse SVD / PCA cases without a GPU: the spectra that make vectors comparable, the structural properties each case is
there for, and the committed tolerances against a fresh measurement (tests/svd_sparse_cases.py)."""
import numpy as np
import pytest

import svd_sparse_cases as sc

pytest.importorskip("scipy.sparse")


@pytest.mark.parametrize("name", sorted(sc.SVD_CASES))
def test_spectrum_and_density(name):
    c = sc.svd_case(name)
    data, k = c["data"].astype(np.float64), c["k"]
    s = np.diag(c["S"])
    lam = np.linalg.eigvalsh(np.dot(data.T, data) if c["left"] else np.dot(data, data.T))[::-1]
    assert np.all(s[:-1] / s[1:] >= 1.05)                      # adjacent kept singular values at least 5 % apart
    kept = s ** 2
    assert kept.min() >= 1e-4 * kept.max() and kept.min() > 1e-4
    if k > 0:
        assert len(s) == k
        full = np.sqrt(np.maximum(lam, 0.0))
        assert full[k - 1] / full[k] >= 1.05                   # ... and the first dropped one
    else:
        assert len(s) == sc.SVD_CASES[name]["blocks"]
        assert np.all(np.abs(lam[len(s):]) < 1e-11)            # dropped eigenvalues far below the 1e-8 cut
    assert np.count_nonzero(data) < 0.25 * data.size, "density"


@pytest.mark.parametrize("name", [n for n in sorted(sc.SVD_CASES) if sc.SVD_CASES[n].get("pert")])
def test_the_perturbation_is_small(name):
    spec = sc.SVD_CASES[name]
    data = sc.dense_data(name).astype(np.float64)
    clean = dict(spec, pert=0)
    sc.SVD_CASES["_clean"] = clean
    try:
        base = sc.dense_data("_clean").astype(np.float64)
    finally:
        del sc.SVD_CASES["_clean"]
        sc._cache.pop(("dense", "_clean"), None)
    k = spec["k"]
    s = spec["smax"] / spec["step"] ** np.arange(k + 1)
    norm = np.linalg.norm(data - base, 2)
    assert 0 < norm < 0.01 * np.min(s[:-1] - s[1:]) and norm < 0.5 * s[k - 1]


def test_structural_properties():
    pad = lambda x: -(-x // 64) * 64
    # LDS or global Gram images, by the padded short side
    assert pad(29) <= sc.GRAM_LDS_MAX_NP and pad(40) <= sc.GRAM_LDS_MAX_NP
    assert pad(130) == 192 > sc.GRAM_LDS_MAX_NP
    # projection panels: 65 kept triples are two panels, the second with one live column; 64 exactly one
    assert pad(sc.SVD_CASES["2100x130_k65"]["k"]) // 64 == 2 and sc.SVD_CASES["2100x130_k65"]["k"] % 64 == 1
    assert sc.SVD_CASES["130x2100_k64"]["k"] == 64
    # a fully dense row, longer than GRAM_CAP and than four 64-entry loads, and a fully dense column
    A = sc.dense_data("130x2100_k64")
    assert np.any(np.count_nonzero(A, axis=1) == 2100) and 2100 > max(sc.GRAM_CAP, 4 * 64)
    assert np.any(np.count_nonzero(A, axis=0) == 130)
    # two empty rows and two empty columns
    B = sc.dense_data("300x40_rank25")
    assert np.sum(np.count_nonzero(B, axis=1) == 0) == 2 and np.sum(np.count_nonzero(B, axis=0) == 0) == 2
    # line counts that are no multiple of the lines a workgroup takes
    assert 37 % sc.PROJ_LINES and 2100 % sc.PROJ_LINES and 300 % sc.PROJ_LINES
    # the input formats describe the same matrix; the coo form holds duplicates
    coo = sc.sparse_data(sc.FORMATS_CASE, "coo_dup")
    assert coo.nnz > sc.sparse_data(sc.FORMATS_CASE).nnz
    for fmt in ("csc", "coo_dup"):
        assert np.array_equal(sc.sparse_data(sc.FORMATS_CASE, fmt).toarray(), sc.dense_data(sc.FORMATS_CASE))


def test_committed_tolerances_match_a_fresh_measurement():
    fresh, stored = sc.measure(), sc.tolerances()
    assert set(fresh) == set(stored) == set(sc.QUANTITIES)
    for q in sc.QUANTITIES:
        assert fresh[q] <= 2.0 * stored[q] + 1e-18 and stored[q] <= 2.0 * fresh[q] + 1e-18, (q, fresh[q], stored[q])
    assert sc.device_tol("U") >= sc.VECTOR_FLOOR and sc.device_tol("ferr2") >= sc.FERR2_FLOOR
