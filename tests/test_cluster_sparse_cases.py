"""The sparse clustering cases without a GPU: the oracle's assignment gaps and member counts, the filled and the emptied lines, the
branch each case is there for (from the constants of the headers, read back), and the committed identity tolerance against a
fresh measurement (tests/cluster_sparse_cases.py)."""
import os
import re

import numpy as np
import pytest

pytest.importorskip("scipy.sparse")

import cluster_oracle as co            # noqa: E402
import cluster_sparse_cases as cs      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymf_amd", "csrc")


def constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


@pytest.mark.parametrize("name", list(cs.SPARSE_CASES))
def test_every_h_step_keeps_the_gap_and_two_members(name):
    r = cs.case(name)["kmeans"]
    print(name, min(r["gaps"]), r["members"], r["ferr"])
    assert len(r["gaps"]) == len(r["members"]) == cs.NITER + 1
    assert min(r["gaps"]) >= cs.MIN_GAP and min(r["members"]) >= 2
    assert len(r["ferr"]) >= 2 and len(cs.case(name)["cmeans"]["ferr"]) >= 2


@pytest.mark.parametrize("name", ["29x300_k5", "151x700_k8"])
def test_the_seed_is_the_first_and_the_run_is_the_oracles(name):
    m, n, k, s, seed = cs.SPARSE_CASES[name]
    assert cs.find_seed(m, n, k, s) == seed
    c = cs.case(name)
    W, H, assigned, ferr, gap = co.kmeans(c["d64"], k, W=c["W0"], niter=cs.NITER)
    r = c["kmeans"]
    assert np.array_equal(W, r["W"]) and np.array_equal(H, r["H"]) and np.array_equal(assigned, r["assigned"])
    assert np.array_equal(ferr, r["ferr"]) and gap == min(r["gaps"])


@pytest.mark.parametrize("name", list(cs.SPARSE_CASES) + [cs.WIDE_CASE])
def test_the_filled_and_the_emptied_lines(name):
    m, n, k, _, _ = cs.shape(name)
    A, W0, _ = cs.planted(*cs.shape(name))
    assert A.has_canonical_format and A.dtype == np.float32 and A.shape == (m, n) and W0.shape == (m, k)
    rows, cols = np.diff(A.indptr), np.diff(A.tocsc().indptr)
    assert rows[m // 3] == n - 2 and cols[n // 3] == m - 2
    assert rows[m // 2] == rows[m - 1] == 0 and cols[n // 2] == cols[0] == 0
    assert np.sum(rows == 0) == 2 and np.sum(cols == 0) == 2 and A.nnz < 0.5 * m * n


def test_the_wide_case_has_a_small_gap():
    c = cs.case(cs.WIDE_CASE)
    print(c["kmeans"]["gap"])
    assert c["kmeans"]["gap"] < cs.MIN_GAP                      # why it is checked sample by sample
    assert np.bincount(c["kmeans"]["assigned"], minlength=3).min() >= 2


def test_the_branches_the_cases_are_there_for():
    assert cs.WAVE == 64 and cs.MIN_LINES == constant("pmf_cluster_csr.h", "PMF_CCSR_MIN_LINES")
    assert cs.CHUNK == constant("pmf_cluster_csr.h", "PMF_CCSR_CHUNK") and cs.MAX_WGS == constant("pmf_cluster.h", "PMF_CL_MAX_WGS")
    sample_len = lambda name: np.diff(cs.case(name)["sparse"].tocsc().indptr)
    # every sample shorter than one load
    assert sample_len("29x300_k5").max() < cs.WAVE
    # the filled sample: two full loads and a tail that ends on one entry; several workgroups, the last ragged
    filled = 151 - 2
    assert sample_len("151x700_k8").max() == filled and filled // cs.WAVE == 2 and (filled % cs.WAVE) % 4 == 1
    assert cs.workgroups(700) == 11 and 700 % cs.lines_per_wg(700) == 60
    assert (300 - 2) % cs.WAVE % 4 == 2 and (80 - 2) % cs.WAVE % 4 == 2 and (1100 - 2) % cs.WAVE % 4 == 2   # ... and on two
    # both widths of the centres, k off the multiples of 16
    ks = sorted(v[2] for v in cs.SPARSE_CASES.values())
    assert ks == [5, 6, 8, 33, 64, 128] and sum(k <= 64 for k in ks) == 5 and cs.WIDE[2] == 3
    # tall data
    assert 1100 > 700
    # the filled row is cut into chunks, raggedly; every other row of these cases fits one chunk or two
    for name, want, last in (("300x5000_k64", 10, 390), ("2100x4100_k128", 9, 2)):
        A = cs.case(name)["sparse"]
        m, n = A.shape
        ch = cs.chunks(A)
        assert ch[m // 3] == want == ch.max() and (n - 2) - (want - 1) * cs.CHUNK == last and ch[m // 2] == 0
        assert last % cs.WAVE % 4 != 0
    assert cs.chunks(cs.case("29x300_k5")["sparse"]).max() == 1
    # more samples than 64 lines x 1024 workgroups
    assert cs.lines_per_wg(66000) == 68 > cs.MIN_LINES and cs.workgroups(66000) == 971 and 66000 % 68 != 0
    for m, n, k, _, _ in cs.SPARSE_CASES.values():
        assert k <= 128 and cs.lines_per_wg(n) == cs.MIN_LINES


def test_committed_tolerances_match_a_fresh_measurement():
    fresh, stored = cs.measure(), cs.tolerances()
    assert set(fresh) == set(stored["measured"]) == set(cs.SPARSE_CASES) and stored["factor"] == cs.FACTOR
    fmax = max(max(v["kmeans"], v["cmeans"]) for v in fresh.values())
    print(fmax, stored["ferr_max"])
    assert fmax <= 2.0 * stored["ferr_max"] and stored["ferr_max"] <= 2.0 * fmax
    assert stored["ferr_max"] == max(max(v["kmeans"], v["cmeans"]) for v in stored["measured"].values())
    for v in stored["measured"].values():                       # rounded up to two digits
        for kind in ("kmeans", "cmeans"):
            assert v[kind] == cs.round_up_2(v[kind])
    assert all(v["kmeans_rel"] >= 0.05 and v["cmeans_rel"] >= 0.05 for v in fresh.values())   # the identity's cancellation stays out
    assert cs.device_tol_ferr() >= 1e-13
