"""The device cases of GREEDY and GREEDYCUR (tests/test_gpu_greedy.py) and what makes the comparison with the float64 oracle
meaningful (tests/test_greedy_cases.py, no GPU): the smallest shapes at which k_greedy_pass, k_greedy_step, k_greedy_gram and
the paths behind them can go wrong.

Data are (randn(m, r) linspace(3, 0.3, r)) randn(r, n) / sqrt(r) with r = min(m, n), float32: a decaying spectrum, so that the
rounds have a clear winner.  Every round of every selection case keeps an argmax gap (best - second) / (best - median) of at
least MIN_GAP in float64 (tests/test_greedy_cases.py asserts it), so the device's float32 products cannot legitimately pick
another column.  Two cases are built by hand: a duplicated column (an exact tie: the lower index wins, the duplicate then
has no residual and scores 0) and data of rank 3 asked for 5 bases.  There the first two rounds keep the gap.  In the third
round the residuals of all columns lie on one line, so every normalised column is the same unit vector up to its sign and all
scores are equal in exact arithmetic: the oracle's scores agree to 1e-9 and its pick is decided by float64 rounding.  The
device's third pick is therefore held to that tie -- a column whose oracle score is the best one to TIE_RTOL -- and not to the
oracle's index.  The rounds behind the rank select on rounding noise in the reference; their indices must be in range.

SELECT_CASES reach branches of the pass and of the Gram-space loop that need wide operands or many panels (what each one is
for stands beside it, and tests/test_greedy_cases.py recomputes it from the constants in the headers).  Only their selection
and W are compared: H and the error over a quarter of a million columns are not what they are for, so their oracle is the
selection and its gaps alone, without H, error or twin.
"""
import numpy as np

import cur_oracle as co
import greedy_oracle as go

MIN_GAP = 1e-3
FACTOR = 4.0             # device tolerance = FACTOR x the oracle-vs-twin deviation
JACOBI_RTOL = 1e-9       # what tests/test_gpu_svd.py holds the float64 Jacobi results to (cur_cases.py)

# name: (rows, cols, num_bases, data seed)
GREEDY_CASES = {
    "5x37_k3": (5, 37, 3, 1),            # one partial panel, rows not a multiple of 4
    "29x300_k6": (29, 300, 6, 2),
    "64x4113_k8": (64, 4113, 8, 3),      # ragged last panel, many workgroups
    "130x1000_k12": (130, 1000, 12, 4),  # two LDS row chunks
    "64x2048_k48": (64, 2048, 48, 5),    # staged operand of 95 columns: six 16-column tiles, every narrower count on the way
    "300x29_k6": (300, 29, 6, 6),        # tall: Gram space
    "2100x64_k12": (2100, 64, 12, 7),    # tall: Gram space
    "80x640_k64": (80, 640, 64, 101),    # operand of 64 .. 127 columns: k_greedy_pass<4> .. <8> in one run, <8> beyond 64 KiB of LDS
}
# selection and W only (see the module docstring): (rows, cols, num_bases, data seed)
SELECT_CASES = {
    "80x2048_k64": (80, 2048, 64, 104),      # the widths of 80x640_k64 on 32 panels: every wave live at eight tiles
    "8x65600_k3": (8, 65600, 3, 148),        # 1025 panels, 2 per workgroup: two live waves; the last workgroup has one panel
    "8x262208_k2": (8, 262208, 2, 138),      # 4097 panels, 5 per workgroup: a second trip of the panel loop, the operand staged once
                                             # (the first seed from 100 on that keeps MIN_GAP)
    "132x262208_k2": (132, 262208, 2, 100),  # the same ranges with two LDS row chunks: the operand staged again on every trip
    "1300x1100_k4": (1300, 1100, 4, 100),    # tall, Gram space with 1100 candidates: threads 0 .. 75 of k_greedy_gram own two
    # the two cases above have their winners among the first four panels of their workgroups (the first trip).  The same data
    # with the columns rotated by ROLL: the scores move with the columns, and the first winner now sits in a fifth panel, so a
    # second trip that lost or spoilt its panel would change the selection
    "8x262208_k2_roll": (8, 262208, 2, 138),
    "132x262208_k2_roll": (132, 262208, 2, 100),
}
ROLL = {"8x262208_k2_roll": 128, "132x262208_k2_roll": 64}
GOLDEN_ONLY = {"37x29_k5": (37, 29, 5, 21)}   # a golden of the reference beyond the device cases (tests/golden/gen_golden_greedy.py)
TIE_CASE = "64x640_k4_tie"               # column TIE_SRC copied to TIE_DUP
RANK_CASE = "29x300_rank3_k5"
RANK = 3
TIE_RTOL = 1e-9          # the spread of the oracle's scores in the round that exhausts the rank (float64 rounding of a tie)
# GREEDYCUR: (rows, cols, rrank, data seed)
GREEDYCUR_CASES = {
    "40x300": (40, 300, 5, 11),          # rows in Gram space, columns by the pass
    "300x40": (300, 40, 5, 12),          # rows by the pass over the transposed copy, columns in Gram space
    "130x2100": (130, 2100, 20, 13),     # two tiles of the Gram matrix, 39 operand columns
    "300x130": (300, 130, 6, 40),        # rows by the pass over a transposed copy of 3 x 5 tiles, columns in Gram space (130 candidates)
}

# The oracle-vs-twin deviations measured on the cases above (tests/test_greedy_cases.py re-measures them and holds them to these
# figures): max |H_twin - H| / max |H| and |ferr_twin - ferr| / ||data||, each with the case that produced it.
TWIN_H_DEV = 6.0e-7          # 300x29_k6 (5.960e-07)
TWIN_FERR_DEV = 2.2e-9       # 80x640_k64 (2.192e-09; 29x300_k6, the largest of the narrower cases: 1.370e-09)
TWIN_CUR_FERR_DEV = 4.4e-10  # GREEDYCUR 40x300 (4.322e-10): W = float32(C U), H = float32(R) through the same residual model


def spectrum_data(rows, cols, seed):
    rng = np.random.RandomState(seed)
    r = min(rows, cols)
    return (np.dot(rng.randn(rows, r) * np.linspace(3.0, 0.3, r), rng.randn(r, cols)) / np.sqrt(r)).astype(np.float32)


def tie_columns(d):
    """(source, duplicate): the winner of the first round and a higher index that receives its copy."""
    src = go.select(d.astype(np.float64), 1)[0]
    return src, (src + 257) % d.shape[1] if (src + 257) % d.shape[1] > src else d.shape[1] - 1


def data(name):
    """float32 data of a case."""
    if name == TIE_CASE:
        d = spectrum_data(64, 640, 8)
        src, dup = tie_columns(d)
        d[:, dup] = d[:, src]
        return d
    if name == RANK_CASE:
        rng = np.random.RandomState(281)    # (the first seed from 9 on whose first two rounds keep MIN_GAP)
        return np.dot(rng.randn(29, RANK), rng.randn(RANK, 300)).astype(np.float32)
    if name in GREEDYCUR_CASES:
        rows, cols, _, seed = GREEDYCUR_CASES[name]
    else:
        rows, cols, _, seed = GREEDY_CASES.get(name) or SELECT_CASES.get(name) or GOLDEN_ONLY[name]
    d = spectrum_data(rows, cols, seed)
    return np.roll(d, ROLL[name], axis=1) if name in ROLL else d


def REPLACED_DATA():
    """29 x 300 data that replace those of 29x300_k6 in place (tests/test_gpu_greedy.py)."""
    return spectrum_data(29, 300, 22)


def num_bases(name):
    return {TIE_CASE: 4, RANK_CASE: 5}.get(name) or (GREEDY_CASES.get(name) or SELECT_CASES[name])[2]


_cache = {}


def case(name):
    """dict(data float32, num_bases, select, gaps, W, H, ferr, twin, scores): the float64 oracle of one GREEDY.factorize() on the
    float32-representable data, and the device model.  A case of SELECT_CASES: dict(data, num_bases, select, gaps, W) alone."""
    if name not in _cache:
        d = data(name)
        d64 = d.astype(np.float64)
        k = num_bases(name)
        gaps, scores = [], []
        sel = go.select(d64, k, gaps=gaps, scores=scores if name == RANK_CASE else None)
        W = d64[:, sel]
        if name in SELECT_CASES:
            _cache[name] = dict(data=d, num_bases=k, select=sel, gaps=gaps, W=W)
            return _cache[name]
        H = go.update_h(d64, W)
        _cache[name] = dict(data=d, num_bases=k, select=sel, gaps=gaps, W=W, H=H, ferr=go.ferr(d64, W, H), twin=go.twin(d, k), scores=scores)
    return _cache[name]


def cur_case(name):
    """dict(data float32, rrank, rid, cid, C, U, R, ferr, twin, tol_U): the float64 oracle of one GREEDYCUR.factorize()."""
    key = ("cur", name)
    if key not in _cache:
        d = data(name)
        d64 = d.astype(np.float64)
        rrank = GREEDYCUR_CASES[name][2]
        gr, gc = [], []
        rid = go.select(d64.T, rrank, gaps=gr)
        cid = go.select(d64, rrank, gaps=gc)
        ones = np.ones(rrank)
        C, U, R = co.compute_ucr(d64, rid, ones, cid, ones)
        gram = co.gram_form(d64, rid, ones, cid, ones)
        kc, kr = float(np.max(gram["kept_c"]) / np.min(gram["kept_c"])), float(np.max(gram["kept_r"]) / np.min(gram["kept_r"]))
        _cache[key] = dict(data=d, rrank=rrank, rid=rid, cid=cid, gaps=gr + gc, C=C, U=U, R=R, ferr=co.ferr(d64, C, U, R),
                           twin=dict(ferr=go.cur_ferr32(d, C, gram["U"], R)), tol_U=(kc + kr) * JACOBI_RTOL)   # tol_U as cur_cases.case
    return _cache[key]


def rel_max(a, b):
    """max |a - b| relative to max |b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def ferr_deviation(c):
    """|ferr(twin) - ferr(oracle)| relative to ||data||."""
    return abs(c["twin"]["ferr"] - c["ferr"]) / float(np.linalg.norm(c["data"].astype(np.float64)))


def h_cases():
    """The cases whose H and ferr are compared: every selection case and the tie case (full column rank W)."""
    return list(GREEDY_CASES) + [TIE_CASE]


def device_tol_h():
    return FACTOR * TWIN_H_DEV


def device_tol_ferr():
    return FACTOR * max(TWIN_FERR_DEV, TWIN_CUR_FERR_DEV)
