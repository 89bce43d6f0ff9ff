"""The device cases of CURSL (tests/test_gpu_cursl.py) and what makes the comparison with the float64 oracle meaningful
(tests/test_cursl_cases.py, no GPU): the smallest shapes at which k_lev_f64, k_lev_gather, k_lev_eig and the host path behind
pmf_cur_leverage can go wrong.

Every case but two has a prescribed spectrum, float32: with rng = RandomState(seed), A = qr(rng.randn(rows, q))[0],
B = qr(rng.randn(cols, q))[0], s = exp(-1.5 arange(q) / q), s[rrank:] *= 0.5, data = sqrt(rows cols / q) (A s) B^T, q = min(rows,
cols).  The leverages are squared norms in the leading kk singular vectors: they are defined up to (eigen-solver error) x
lambda_kk / (lambda_kk - lambda_kk+1), and plain uniform data has s_k / s_k+1 = 1.0004 at the cut -- the leverages would hinge
on how Jacobi splits a near-degenerate pair.  The halved tail puts a factor 4 between lambda_kk and lambda_kk+1.
`29x300_full` is plain rand(29, 300): k = 40 is beyond the rank, all 29 vectors are taken and no gap is involved; `doc_2x3`
is cursl.py's own example.

k_lev_f64 gives a wave 64 positions of the long side and a workgroup 256, walks the short side in pieces of 64 and takes
ceil(kk / 16) operand tiles; the comments in the table name what each case reaches there.
"""
import json
import os

import numpy as np

import cur_cases as cc
import cur_oracle as co
import cursl_oracle as cso

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "golden", "cursl_tolerances.json")

# name: (rows, cols, rrank, data kind, data seed, draw seed)
CURSL_CASES = {
    "doc_2x3": (2, 3, 1, "doc", 0, 11),                        # cursl.py:57-59
    "37x29": (37, 29, 5, "spectrum", 71, 21),                  # tall (TRANS = false); kk not a multiple of 16; one panel
    "29x300": (29, 300, 6, "spectrum", 72, 22),                # wide (TRANS = true); q padded 29 -> 64; two workgroups, the second with one wave
    "29x300_full": (29, 300, 40, "uniform", 73, 23),           # k beyond the rank: kk = 29; repeated columns of rank-29 data: C^T C has null eigenvalues
    "29x2100": (29, 2100, 20, "spectrum", 74, 24),             # 33 panels of 64, ragged np = 2112: nine workgroups, the last with one wave
    "130x2100": (130, 2100, 70, "spectrum", 75, 25),           # kk > 64: five operand tiles; q = 130 padded to 192: three pieces
    "2100x130": (2100, 130, 70, "spectrum", 76, 26),           # the TRANS = false mirror
    "200x200": (200, 200, 128, "spectrum", 77, 27),            # the limit: eight operand tiles; rows <= cols at equality
    "300x2432": (300, 2432, 16, "spectrum", 80, 30),           # an inner dimension of five 64-blocks; one operand tile
}

MAX_K = 128              # PMF_LEV_MAX_K (pymf_amd/csrc/pmf_lev.h)
MARGIN_FACTOR = 100.0    # every draw is at least this many tol_cum away from every cumulative sum

_DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])


def spectrum_data(rows, cols, rrank, seed):
    """float32 data with the prescribed spectrum of the module docstring."""
    rng = np.random.RandomState(seed)
    q = min(rows, cols)
    A = np.linalg.qr(rng.randn(rows, q))[0]
    B = np.linalg.qr(rng.randn(cols, q))[0]
    s = np.exp(-1.5 * np.arange(q) / q)
    s[rrank:] *= 0.5
    return (np.sqrt(rows * cols / float(q)) * np.dot(A * s, B.T)).astype(np.float32)


def data(name):
    """float32 data of a case."""
    rows, cols, rrank, kind, seed, _ = CURSL_CASES[name]
    if kind == "doc":
        return _DOC.astype(np.float32)
    if kind == "uniform":
        return np.random.RandomState(seed).rand(rows, cols).astype(np.float32)
    return spectrum_data(rows, cols, rrank, seed)


_cache = {}


def case(name):
    """dict of the float64 oracle of one CURSL.factorize() on the float32-representable data: data, rrank, seed, the ranks
    k_rows / k_cols handed to the leverages and their kk, lev_r / lev_c (unnormalised), prow / pcol, g and tol_cum, the draws
    with their margins, and C, U, R, ferr, gram, twin, kappa_c, kappa_r, tol_U as cur_cases.case."""
    if name not in _cache:
        d = data(name)
        d64 = d.astype(np.float64)
        rrank, seed = CURSL_CASES[name][2], CURSL_CASES[name][5]
        nr, nc = cso.ranks(d64, rrank)
        lev_c, kk_c, lam = cso.leverage(d64, nr)               # cursl.py:87: the columns with _rrank
        lev_r, kk_r, _ = cso.leverage(d64.T, nc)               # cursl.py:88: the rows with _crank
        g = max(cso.gap_factor(lam, kk_c), cso.gap_factor(lam, kk_r))
        margins = []
        rid, cid, rcnt, ccnt, prow, pcol = cso.draw(d64, rrank, seed, margins=margins)
        C, U, R = co.compute_ucr(d64, rid, rcnt, cid, ccnt)
        gram = co.gram_form(d64, rid, rcnt, cid, ccnt)
        kc, kr = cc.cond(gram["kept_c"]), cc.cond(gram["kept_r"])
        _cache[name] = dict(data=d, rrank=rrank, seed=seed, k_rows=nc, k_cols=nr, kk_r=kk_r, kk_c=kk_c, lev_r=lev_r, lev_c=lev_c,
                            lam=lam, prow=prow, pcol=pcol, g=g, tol_cum=cc.JACOBI_RTOL * g, margins=margins,
                            rid=rid, cid=cid, rcnt=rcnt, ccnt=ccnt, C=C, U=U, R=R, ferr=co.ferr(d64, C, U, R), gram=gram,
                            twin=co.twin(d64, rid, rcnt, cid, ccnt), kappa_c=kc, kappa_r=kr, tol_U=(kc + kr) * cc.JACOBI_RTOL)
    return _cache[name]


def measure():
    """Per case: kappa_c, kappa_r, tol_U, tol_cum and the twin's ferr deviation."""
    out = {}
    for name in CURSL_CASES:
        c = case(name)
        out[name] = dict(kappa_c=c["kappa_c"], kappa_r=c["kappa_r"], tol_U=c["tol_U"], tol_cum=c["tol_cum"], ferr=cc.ferr_deviation(c))
    return out


def tolerances():
    """The committed figures (tests/golden/cursl_tolerances.json, written by tests/golden/gen_golden_cursl.py)."""
    with open(TOL_PATH) as f:
        return json.load(f)


def device_tol_ferr():
    """cur_cases.FACTOR x the largest oracle-vs-twin deviation of the error over all cases."""
    return cc.FACTOR * tolerances()["ferr_max"]
