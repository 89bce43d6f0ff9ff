"""The sparse GREEDY cases without a GPU: the oracle's argmax gaps, the emptied lines, the branch each case is there for (from the
constants of the headers), the committed identity tolerance against a fresh measurement, and the goldens of the reference's own
sparse branch (tests/greedy_sparse_cases.py)."""
import os
import re

import numpy as np
import pytest

pytest.importorskip("scipy.sparse")

import greedy_cases as gc             # noqa: E402
import greedy_sparse_cases as gs      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymf_amd", "csrc")


def constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


@pytest.mark.parametrize("name", list(gs.SPARSE_CASES))
def test_every_round_keeps_the_gap(name):
    c = gs.case(name)
    print(name, min(c["gaps"]), c["select"][:8])
    assert len(c["gaps"]) == c["num_bases"] and min(c["gaps"]) >= gc.MIN_GAP
    if name in gs.TRANSPOSED:
        assert len(c["gaps_t"]) == c["num_bases"] and min(c["gaps_t"]) >= gc.MIN_GAP


@pytest.mark.parametrize("name", list(gs.SPARSE_CASES))
def test_the_emptied_lines_have_zero_norm_and_are_not_selected(name):
    c = gs.case(name)
    m, n = c["data"].shape
    rows, cols = gs.empty_lines(m, n)
    assert all(np.all(c["data"][r, :] == 0) for r in rows) and all(np.all(c["data"][:, q] == 0) for q in cols)
    assert np.sum(np.count_nonzero(c["data"], axis=1) == 0) == 2 and np.sum(np.count_nonzero(c["data"], axis=0) == 0) == 2
    assert not set(c["select"]) & set(cols)
    if name in gs.TRANSPOSED:
        assert not set(c["select_t"]) & set(rows)
    assert np.count_nonzero(c["data"][:, n // 3]) == m - 2 and np.count_nonzero(c["data"][m // 3, :]) == n - 2
    assert c["sparse"].has_canonical_format and c["sparse"].dtype == np.float32


def test_the_tie_and_the_rank_case():
    c = gs.case(gs.TIE_CASE)
    m, n, _, density, seed = gs.TIE_BASE
    src, dup = gs.tie_columns(gs.raw_matrix(m, n, density, seed).toarray())
    assert dup > src and np.array_equal(c["data"][:, src], c["data"][:, dup])
    assert c["select"][0] == src and dup not in c["select"] and min(c["gaps"][1:]) >= gc.MIN_GAP
    r = gs.case(gs.RANK_CASE)
    s = np.linalg.svd(r["data"].astype(np.float64), compute_uv=False)
    assert s[gs.RANK - 1] > 1e-2 * s[0] and s[gs.RANK] < 1e-6 * s[0]          # rank 3 up to the float32 rounding of the entries
    assert min(r["gaps"][:gs.RANK - 1]) >= gc.MIN_GAP
    T = r["scores"][gs.RANK - 1]
    assert np.sum(T >= T.max() * (1.0 - gc.TIE_RTOL)) > 1                     # the third round is a tie
    assert np.count_nonzero(r["data"]) < r["data"].size


def test_the_branches_the_cases_are_there_for():
    assert gs.WAVE == 64 and gs.MIN_LINES == constant("pmf_greedy_csr.h", "PMF_GCSR_MIN_LINES")
    assert gs.MAX_WGS == constant("pmf_cluster.h", "PMF_CL_MAX_WGS")
    pad = lambda x: -(-x // 64) * 64
    assert gs.GRAM_MAX_NP == constant("pmf_host_snmf.h", "PMF_GRAM_MAX_NP")
    # wide under 64 rows: no line reaches a second load
    assert gs.wide("29x300_k6") and 29 < gs.WAVE
    # the filled column: a third trip of the entry loop and a tail of one entry; several workgroups, the last ragged
    filled = 151 - 2
    assert gs.wide("151x700_k8") and filled > 2 * gs.WAVE and (filled % gs.WAVE) % 4 == 1
    assert gs.workgroups(700) == 11 and 700 % gs.lines_per_wg(700) == 60
    # both lane forms in one run: the operand grows from c to c + 63 columns
    c = gs.case("80x640_k64")
    rank = int(np.sum(np.linalg.eigvalsh(np.dot(c["data"].astype(np.float64), c["data"].astype(np.float64).T)) > 1e-8))
    cc = min(64, rank)
    assert gs.wide("80x640_k64") and cc <= 64 < cc + 63 <= 127
    # more candidates than 64 lines x 1024 workgroups
    assert gs.lines_per_wg(66000) == 68 > gs.MIN_LINES and gs.workgroups(66000) == 971 and 66000 % 68 != 0
    # Gram space, the square case on the pass, the limit
    assert not gs.wide("300x29_k6") and not gs.wide("2100x64_k12") and gs.wide("200x200_k10")
    assert pad(1000) == gs.GRAM_MAX_NP and gs.wide("1000x1100_k4")
    for name, (m, n, k, _, _) in gs.SPARSE_CASES.items():
        assert min(pad(m), pad(n)) <= gs.GRAM_MAX_NP and k <= 64


def test_committed_tolerances_match_a_fresh_measurement():
    fresh, stored = gs.measure(), gs.tolerances()
    assert set(fresh) == set(stored["measured"]) == set(gs.h_cases())
    fmax = max(v["ferr"] for v in fresh.values())
    print(fmax, stored["ferr_max"])
    assert fmax <= 2.0 * stored["ferr_max"] and stored["ferr_max"] <= 2.0 * fmax
    assert stored["ferr_max"] == max(v["ferr"] for v in stored["measured"].values())
    assert all(v["ferr_rel"] >= 0.05 for v in fresh.values())                  # the identity's cancellation stays out of the comparison
    assert gs.device_tol_ferr() >= 1e-13


@pytest.mark.parametrize("name", ["29x300_k6", "300x29_k6"])
def test_the_reference_sparse_branch_agrees_with_the_oracle(name):
    """tests/golden/greedy_sparse_<case>.npz: `select` of the reference's own sparse branch (greedy.py:115-141 on a csc_matrix)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "greedy_sparse_%s.npz" % name))
    assert str(g["case"]) == name and [int(s) for s in g["select"]] == gs.case(name)["select"]
