"""The device cases of CUR and CMD (tests/test_gpu_cur.py) and what makes the comparison with the float64 oracle meaningful
(tests/test_cur_cases.py, no GPU): the smallest shapes at which k_cur_sqnorms, k_cur_gather, k_prod_f64 (full tile grid) and the paths
behind them can go wrong.

"Low rank" data are rand(m, 12) rand(12, n) + 0.05 rand(m, n), "uniform" data plain rand(m, n), both float32.  Every case runs
as CUR and, with the same seed, as CMD.  The cross product cuts the inner dimension as the Gram matrix does (one kernel, k_prod_f64: svd_cases.chunks): 300
columns (padded to 320) are one chunk, 2 100 (padded to 2 112) four chunks of 576 with a ragged tail of 384.  With 70 draws
from 130 rows a repeated index is as good as certain (tests/test_cur_cases.py asserts that the seeds at hand have them), so
CUR's Gram matrices there are singular -- a null eigenvalue must be dropped -- and CMD's counts exceed 1.
"""
import json
import os

import numpy as np

import cur_oracle as co

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "golden", "cur_tolerances.json")

# name: (rows, cols, rrank, data kind, data seed, draw seed)
CUR_CASES = {
    "doc_2x3": (2, 3, 1, "doc", 0, 11),                        # cur.py:54-56
    "37x29": (37, 29, 5, "lowrank", 61, 12),                   # tall (TRANS = true), odd sizes, one tile, one chunk
    "29x300": (29, 300, 6, "lowrank", 62, 13),                 # wide, one tile, one chunk
    "29x2100": (29, 2100, 20, "uniform", 63, 14),              # wide, four chunks with a ragged tail
    "130x2100": (130, 2100, 70, "uniform", 64, 15),            # wide, two tiles in both output dimensions, two row blocks of the norms pass, duplicates
    "2100x130": (2100, 130, 70, "uniform", 65, 16),            # the TRANS = true mirror
    "200x200": (200, 200, 128, "uniform", 66, 17),             # the limit; rows <= cols at equality
}
KINDS = ("cur", "cmd")

MAX_RANK = 128           # PMF_CUR_MAX_RANK (pymf_amd/csrc/pmf_cur.h)
FACTOR = 4.0             # device tolerance of the error = FACTOR x the oracle-vs-twin deviation
JACOBI_RTOL = 1e-9       # what tests/test_gpu_svd.py holds the float64 Jacobi results to

_DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])


def data(name):
    """float32 data of a case."""
    rows, cols, _, kind, seed, _ = CUR_CASES[name]
    if kind == "doc":
        return _DOC.astype(np.float32)
    rng = np.random.RandomState(seed)
    if kind == "lowrank":
        return (np.dot(rng.rand(rows, 12), rng.rand(12, cols)) + 0.05 * rng.rand(rows, cols)).astype(np.float32)
    return rng.rand(rows, cols).astype(np.float32)


def cond(kept):
    return float(np.max(kept) / np.min(kept))


_cache = {}


def case(name, kind):
    """dict(data float32, rrank, seed, rid, cid, rcnt, ccnt, margins, C, U, R, ferr, gram, twin, kappa_c, kappa_r, tol_U): the
    float64 oracle of one CUR.factorize() (kind "cur") or CMD.factorize() ("cmd") on the float32-representable data."""
    if (name, kind) not in _cache:
        d = data(name)
        d64 = d.astype(np.float64)
        rrank, seed = CUR_CASES[name][2], CUR_CASES[name][5]
        margins = []
        rid, cid, rcnt, ccnt = co.draw(d64, rrank, seed, cmd=(kind == "cmd"), margins=margins)
        C, U, R = co.compute_ucr(d64, rid, rcnt, cid, ccnt)
        gram = co.gram_form(d64, rid, rcnt, cid, ccnt)
        kc, kr = cond(gram["kept_c"]), cond(gram["kept_r"])
        _cache[(name, kind)] = dict(data=d, rrank=rrank, seed=seed, rid=rid, cid=cid, rcnt=rcnt, ccnt=ccnt, margins=margins,
                                    C=C, U=U, R=R, ferr=co.ferr(d64, C, U, R), gram=gram,
                                    twin=co.twin(d64, rid, rcnt, cid, ccnt), kappa_c=kc, kappa_r=kr,
                                    tol_U=(kc + kr) * JACOBI_RTOL)
    return _cache[(name, kind)]


def rel_max(a, b):
    """max |a - b| relative to max |b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def ferr_deviation(c):
    """|ferr(twin) - ferr(oracle)| relative to ||data||."""
    return abs(c["twin"]["ferr"] - c["ferr"]) / float(np.linalg.norm(c["data"].astype(np.float64)))


def measure():
    """Per case and kind: kappa_c, kappa_r, tol_U and the twin's ferr deviation."""
    out = {}
    for name in CUR_CASES:
        for kind in KINDS:
            c = case(name, kind)
            out["%s_%s" % (kind, name)] = dict(kappa_c=c["kappa_c"], kappa_r=c["kappa_r"], tol_U=c["tol_U"], ferr=ferr_deviation(c))
    return out


def tolerances():
    """The committed figures (tests/golden/cur_tolerances.json, written by tests/golden/gen_golden_cur.py)."""
    with open(TOL_PATH) as f:
        return json.load(f)


def device_tol_ferr():
    """FACTOR x the largest oracle-vs-twin deviation of the error over all cases (as svd_cases.device_tol)."""
    return FACTOR * tolerances()["ferr_max"]
