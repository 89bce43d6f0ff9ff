"""The device cases of GREEDY on scipy.sparse data (tests/test_gpu_greedy_sparse.py) and what makes the comparison with the
float64 oracle on toarray() meaningful (tests/test_greedy_sparse_cases.py, no GPU): the smallest shapes at which
k_greedy_csr_pass, k_greedy_step_csr, k_greedy_csr_gather, the Gram-space loop on the CSR Gram matrix and the H step can go wrong.

Data: scipy.sparse.random(m, n, density, random_state=RandomState(seed)) with values 0.25 + rand, the rows scaled by
linspace(3, 0.3, m) so that the rounds have a winner, float32.  Then, as in tests/cur_sparse_cases.py, row m // 3 and column
n // 3 are filled completely (the long lines) and after that rows m // 2 and m - 1 and columns n // 2 and 0 are emptied: their
norms are exactly 0, they score 0 and must never be selected.  The filled column has m - 2 entries.

The yardstick is tests/greedy_oracle.py in float64 on toarray().  Every round of every case keeps greedy_cases.MIN_GAP
(tests/test_greedy_sparse_cases.py asserts it); the seed of a case is the first one from the start stated beside it that does.
The tie case and the rank case are built by hand as in tests/greedy_cases.py and held the same way.

ferr on sparse data is the identity ferr^2 = ||data||^2 - 2 <W^T data, H> + <W^T W, H H^T> in float64.  Its deviation from the
direct norm on the oracle's factors, relative to ||data||, is what the identity's cancellation is worth on these data; the device
is held to FACTOR x the worst of them, floored at cur_sparse_cases.FERR_FLOOR (tests/golden/greedy_sparse_tolerances.json).
"""
import json
import os

import numpy as np
import scipy.sparse as sp

import greedy_cases as gc
import greedy_oracle as go

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "golden", "greedy_sparse_tolerances.json")

# constants of the headers that decide which branch a case reaches (tests/test_greedy_sparse_cases.py reads them back)
WAVE = 64                # entries a wave of k_greedy_csr_pass loads at a time
MIN_LINES = 64           # PMF_GCSR_MIN_LINES: lines per workgroup at least
MAX_WGS = 1024           # PMF_CL_MAX_WGS: partials
GRAM_MAX_NP = 1024       # PMF_GRAM_MAX_NP: the short side, padded to 64

# name: (rows, cols, num_bases, density, data seed); every seed is the first from 1 on that keeps MIN_GAP in every round (and, for
# the cases of TRANSPOSED, in every round of the selection on toarray().T as well)
SPARSE_CASES = {
    "29x300_k6": (29, 300, 6, 0.2, 2),           # wide, under 64 rows: every line shorter than one load
    "151x700_k8": (151, 700, 8, 0.05, 1),        # wide; the filled column has 149 = 2 * 64 + 21 entries: a third trip of the entry
                                                 # loop and a one-entry tail; 11 workgroups, the last with 60 lines
    "80x640_k64": (80, 640, 64, 0.3, 1),         # c + i crosses 64: k_greedy_csr_pass<1> and <2> in one run
    "12x66000_k3": (12, 66000, 3, 0.3, 6),       # more than 64 * 1024 candidates: 68 lines per workgroup, 971 workgroups, the last ragged
    "300x29_k6": (300, 29, 6, 0.2, 2),           # tall: Gram space on the CSR Gram matrix
    "2100x64_k12": (2100, 64, 12, 0.05, 2),      # tall: Gram space, one full tile of candidates
    "200x200_k10": (200, 200, 10, 0.1, 1),       # rows = cols: the pass over stored entries, not Gram space
    "1000x1100_k4": (1000, 1100, 4, 0.01, 1),    # the short side pads to 1024, the limit
}
TRANSPOSED = ("300x29_k6", "29x300_k6")          # pmf_greedy_select(transposed = 1): the pass over the image of V / Gram space
TIE_CASE = "64x640_k4_tie"
TIE_BASE = (64, 640, 4, 0.2, 1)          # (seed 1: the rounds behind the planted tie keep MIN_GAP)
RANK_CASE = "29x300_rank3_k5"
RANK_SEED = 3            # the first seed from 1 on whose first two rounds keep MIN_GAP
RANK = gc.RANK
FACTOR = gc.FACTOR


def raw_matrix(m, n, density, seed):
    rng = np.random.RandomState(seed)
    A = sp.random(m, n, density=density, random_state=rng, data_rvs=lambda k: 0.25 + rng.rand(k), dtype=np.float64).tolil()
    A[m // 3, :] = 0.25 + rng.rand(n)
    A[:, n // 3] = (0.25 + rng.rand(m)).reshape(m, 1)
    for r in (m // 2, m - 1):
        A[r, :] = 0.0
    for c in (n // 2, 0):
        A[:, c] = 0.0
    A = sp.diags(np.linspace(3.0, 0.3, m)).dot(A.tocsr()).tocsr().astype(np.float32)
    A.eliminate_zeros()
    A.sum_duplicates()
    return A


def empty_lines(m, n):
    """(rows, cols) emptied by raw_matrix."""
    return (m // 2, m - 1), (n // 2, 0)


def tie_columns(d):
    return gc.tie_columns(d)


def matrix(name):
    """The case's data as a canonical float32 csr_matrix."""
    if name == TIE_CASE:
        m, n, _, density, seed = TIE_BASE
        d = raw_matrix(m, n, density, seed).toarray()
        src, dup = tie_columns(d)
        d[:, dup] = d[:, src]
        return sp.csr_matrix(d)
    if name == RANK_CASE:
        rng = np.random.RandomState(RANK_SEED)
        A = rng.randn(29, RANK)
        A[[14, 28], :] = 0.0
        B = rng.randn(RANK, 300) * (rng.rand(RANK, 300) < 0.6)
        return sp.csr_matrix(np.dot(A, B).astype(np.float32))
    m, n, _, density, seed = SPARSE_CASES[name]
    return raw_matrix(m, n, density, seed)


def num_bases(name):
    return {TIE_CASE: TIE_BASE[2], RANK_CASE: 5}.get(name) or SPARSE_CASES[name][2]


def identity_ferr(d64, W, H):
    """The trace identity of the module docstring in float64, ||data||^2 as the sum of the row norms."""
    vn = float(np.sum(np.sum(d64 ** 2, axis=1)))
    f2 = vn - 2.0 * float(np.sum(np.dot(W.T, d64) * H)) + float(np.sum(np.dot(W.T, W) * np.dot(H, H.T)))
    return float(np.sqrt(max(f2, 0.0)))


_cache = {}


def case(name):
    """dict(sparse csr float32, data dense float32, num_bases, select, gaps, scores, W, H, ferr, ferr_twin, norm): the float64 oracle
    of one GREEDY.factorize() on toarray().  A case of TRANSPOSED also has select_t, gaps_t: the selection on toarray().T."""
    if name not in _cache:
        A = matrix(name)
        d = A.toarray()
        d64 = d.astype(np.float64)
        k = num_bases(name)
        gaps, scores = [], []
        sel = go.select(d64, k, gaps=gaps, scores=scores if name == RANK_CASE else None)
        W = d64[:, sel]
        c = dict(sparse=A, data=d, num_bases=k, select=sel, gaps=gaps, scores=scores, W=W, norm=float(np.linalg.norm(d64)))
        if name != RANK_CASE:                             # (full column rank W)
            H = go.update_h(d64, W)
            c.update(H=H, ferr=go.ferr(d64, W, H), ferr_twin=identity_ferr(d64, W, H))
        if name in TRANSPOSED:
            gt = []
            c.update(select_t=go.select(d64.T.copy(), k, gaps=gt), gaps_t=gt)
        _cache[name] = c
    return _cache[name]


def h_cases():
    return list(SPARSE_CASES) + [TIE_CASE]


def twin_deviation(c):
    """|identity - direct| of the oracle's error, relative to ||data||."""
    return abs(c["ferr_twin"] - c["ferr"]) / c["norm"]


def measure():
    out = {name: dict(ferr=twin_deviation(case(name)), ferr_rel=case(name)["ferr"] / case(name)["norm"]) for name in h_cases()}
    return out


def tolerances():
    """The committed figures (tests/golden/greedy_sparse_tolerances.json, written by tests/golden/gen_golden_greedy_sparse.py)."""
    with open(TOL_PATH) as f:
        return json.load(f)


def device_tol_ferr():
    """FACTOR x the largest identity-vs-direct deviation over all cases, floored at cur_sparse_cases.FERR_FLOOR."""
    import cur_sparse_cases as csc
    return max(FACTOR * tolerances()["ferr_max"], csc.FERR_FLOOR)


# ---- which branch a case reaches, from the constants above ---------------------------------------------------------------------
def wide(name):
    m, n = SPARSE_CASES[name][:2]
    return m <= n


def lines_per_wg(cands):
    return -(-max(MIN_LINES, -(-cands // MAX_WGS)) // 4) * 4


def workgroups(cands):
    return -(-cands // lines_per_wg(cands))
