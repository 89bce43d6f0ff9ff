"""The conditions under which the device comparison of tests/test_gpu_sivm_sparse.py means something, on the oracles alone (no
GPU): a clear argmax at every selection step, the float32 sparse-form twin selecting what the float64 oracle selects on
toarray(), a well-conditioned W^T W and a multiplier search inside the device's cap where H is compared, the float32 deviation
the H tolerance is made of, and the committed goldens -- the real reference on toarray() -- equal to the oracle."""
import numpy as np
import pytest
import scipy.sparse as sp

import sivm_cases as sc
import sivm_oracle as so
import sivm_sparse_cases as ssc
import sivm_sparse_oracle as sso
from conftest import load_golden

COMBOS = ssc.combos(ssc.CASES) + ssc.combos(ssc.PANEL_CASES)
BIG = []
H_COMBOS = [p for p in COMBOS if ssc.has_h(*p)]
GOLDEN = {"sivm_sparse_%s_%s" % (n, m): (n, "sivm", m, "fastmap") for n in ("5x37_k3", "29x300_k6_empty", "29x300_k6", "31x300_k6")
          for m in ssc.METRICS if (n, m) != ("29x300_k6_empty", "cosine")}
CSC_RUN_AGREES = ("5x37_k3", "29x300_k6_empty")              # (gen_golden_sivm_sparse.py: elsewhere the reference's CSC run picks a column twice)


def ident(p):
    return "-".join(p)


@pytest.mark.parametrize("p", COMBOS + BIG, ids=ident)
def test_gap_twin_and_condition(p):
    name, rule, metric, init = p
    g, same, cond = ssc.conditions(*p)
    c = ssc.case(*p)
    assert ssc.holds(*p)
    assert g >= sc.MIN_GAP, "gap %.2e" % g
    assert same, "the float32 sparse-form twin selects otherwise"
    if (name, metric) == ("29x300_k6_empty", "cosine"):
        assert set(c["select"]) <= {-1, 0}                     # every cosine distance to the origin or to the empty column 0 is exactly 1: column 0 wins every tie
    else:
        assert len(set(c["select"])) == c["k"]                 # (no column twice: the reference's NaN re-pick does not occur)
    if ssc.has_h(*p):
        assert cond <= sc.MAX_COND
    if c["special"] in ("ends", "trip2") and init == "fastmap" and metric == "l2":
        assert min(c["select"]) < 64 and max(c["select"]) >= c["csc"].shape[1] - 64
    if c["special"] == "trip2":
        assert sc.TRIP2_COLUMN in c["select"]


@pytest.mark.parametrize("p", ssc.NO_SEED, ids=ident)
def test_the_combinations_without_a_seed_have_none_among_the_first(p):
    """NO_SEED: the search that chose every other seed fails for these (its first 20 seeds here; 150 when the list was made),
    and it is the argmax gap that fails.  They are the only combinations of the tables that the device tests leave out."""
    assert p[0] in ssc.CASES and p[1:] in ssc.CASES[p[0]][6] and p not in ssc.SEEDS
    assert ssc.find_seed(p[0], p[1:], tries=20) is None
    assert ssc.conditions(*p)[0] < sc.MIN_GAP
    assert len(ssc.NO_SEED) == 4 and {q[0] for q in ssc.NO_SEED} == {"64x2048_k64"}


def test_every_listed_combination_runs_or_is_in_no_seed():
    for table in (ssc.CASES, ssc.PANEL_CASES):
        for name, c in table.items():
            assert c[6] == ssc.ALL or name == "8x1048592_k3"    # (one million columns: the two 'l2' 'fastmap' runs, as sivm_cases.PANEL_CASES)
    assert len(COMBOS) == 9 * 12 + 2 - len(ssc.NO_SEED)


def test_the_tie_is_a_tie_and_the_empty_columns_are_empty():
    c = ssc.case("16x640_k4_tie")
    assert np.array_equal(c["V"][:, 70], c["V"][:, 600])
    assert 70 in c["select"] and 600 not in c["select"]
    assert any(np.sort(s)[-1] == np.sort(s)[-2] for s in c["scores"])
    e = ssc.case("29x300_k6_empty")["csc"]
    lens = np.diff(e.indptr)
    assert all(lens[col] == 0 for col in ssc.EMPTY_COLUMNS) and lens[0] == 0 and lens[-1] == 0
    W = ssc.case("29x300_k6_empty", "sivm", "l2", "origin")["W"]
    assert not W[:, 0].any()                                   # -1 reads the empty last column


def test_the_row_limit_case_is_at_the_limit_and_sparse():
    csc = ssc.data("16384x1000_k6")[0]
    assert csc.shape[0] == 16384 and csc.nnz / float(csc.shape[0] * csc.shape[1]) < 0.01


def test_clamp_and_self_distance_of_the_sparse_form():
    """what the twin is for: the expansion-form sums leave rounding noise where the difference form gives 0"""
    csc = ssc.data("64x4113_k8")[0]
    V = csc.toarray().astype(np.float64)
    for metric in ("l2", "l1"):
        for idx in (3, 1004, 4111):
            d = sso.distance32(csc, idx, metric)
            assert d[idx] == 0.0 and d.min() >= 0.0
            ref = so.distance(V, idx, metric)
            assert np.abs(d - ref).max() <= 2e-5 * ref.max()
    twin = sp.csc_matrix(np.array([[3.0, 3.0], [0.1, 0.1000001]], dtype=np.float32))
    assert sso.distance32(twin, 0, "l2")[1] >= 0.0             # (clamped: never the sqrt of a negative sum)
    assert np.all(sso.distance32(csc, -1, "cosine") == 1.0)


@pytest.mark.parametrize("p", H_COMBOS, ids=ident)
def test_rounds_and_fp32_deviation(p):
    c = ssc.case(*p)
    V64 = c["V"].astype(np.float64)
    _, _, S, F = so.products(V64, c["W"], True, True, True)
    Hr, rounds = so.simplex_rounds(S, F)
    assert rounds.max() <= sc.ROUND_CAP // 2, "%d rounds" % rounds.max()
    H = ssc.h_oracle(*p)[0]
    H32, _ = so.update_h(V64, c["W"], True, True, True, True)
    dh = np.linalg.norm(H32 - H) / np.linalg.norm(H)
    print("%s: H deviation %.3e, rounds max %d" % (ident(p), dh, rounds.max()))
    assert dh <= ssc.MEASURED_H_SPARSE * 1.001                 # the figure H_TOL is made of


@pytest.mark.parametrize("gname", sorted(GOLDEN))
def test_goldens_equal_the_oracle(gname):
    g = load_golden(gname)
    p = GOLDEN[gname]
    c = ssc.case(*p)
    csc = c["csc"]
    assert np.array_equal(g["indptr"], csc.indptr) and np.array_equal(g["indices"], csc.indices) and np.array_equal(g["data"], csc.data)
    assert g["select"].tolist() == c["select"]
    assert np.array_equal(g["W"], c["W"])
    assert np.abs(g["H"] - ssc.h_oracle(*p)[0]).max() <= 1e-9
    if str(g["metric"]) == "l2":
        assert bool(g["csc_run_agrees"]) == (p[0] in CSC_RUN_AGREES)
        if p[0] in CSC_RUN_AGREES:
            assert g["select_csc"].tolist() == c["select"]
        else:
            assert len(set(g["select_csc"].tolist())) < c["k"]       # the NaN re-pick: a column twice
