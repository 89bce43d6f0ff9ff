"""The device cases of CUR and CMD on scipy.sparse data (tests/test_gpu_cur_sparse.py) and what makes the comparison with the
float64 oracle on toarray() meaningful (tests/test_cur_sparse_cases.py, no GPU): the smallest shapes at which
k_cur_csr_sqnorms, k_cur_csr_gather and k_cur_csr_mid can go wrong.

Data: scipy.sparse.random(m, n, density, random_state=RandomState(seed)) with values 0.25 + rand, float32.  Then row m // 3
and column n // 3 are filled completely (the long lines: longer than a team of the norms pass, and in 3000 x 2500 and
1100 x 4100 longer than one 256-entry chunk of the middle product), and after that rows m // 2 and m - 1 and columns n // 2
and 0 are emptied (so the long lines miss those two crossings, and the empty lines are exactly empty: their norms are 0,
they are never drawn).  Every case runs as CUR and, with the same seed, as CMD; the draw seed is 100 + the data seed.

frobenius_norm on sparse data is the identity  ferr^2 = ||data||^2 - 2 <U, C^T data R^T> + <(C^T C) U, U (R R^T)>.  Its "twin"
here is that identity in NumPy float64 on the oracle's C, U, R; its deviation from the direct cur_oracle.ferr, relative to
||data||, is what the summation order of the identity is worth, and the device is held to FACTOR x the worst of them (floored
at 1e-13; tests/golden/cur_sparse_tolerances.json).  The dense device run on toarray() evaluates the error by a float32
residual pass instead; cur_oracle.twin models it, and the two device runs may differ by FACTOR x the worst deviation of that
twin from the oracle on these data plus the sparse run's own tolerance.
"""
import json
import os

import numpy as np
import scipy.sparse as sp

import cur_cases as cc
import cur_oracle as co

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "golden", "cur_sparse_tolerances.json")

# name: (rows, cols, rrank, density, data seed)
SPARSE_CASES = {
    "37x29": (37, 29, 5, 0.3, 1),                              # small tall data
    "29x300": (29, 300, 6, 0.2, 2),                            # small wide data
    "130x2100": (130, 2100, 70, 0.05, 3),                      # repeated draws; more than one 64-wide tile
    "2100x130": (2100, 130, 70, 0.05, 4),                      # the mirror
    "200x200": (200, 200, 128, 0.2, 5),                        # the rank limit
    "3000x2500": (3000, 2500, 64, 0.01, 6),                    # exactly one tile
    "1100x4100": (1100, 4100, 65, 0.004, 7),                   # one past a tile; very short lines beside the long ones
}
KINDS = cc.KINDS
FERR_FLOOR = 1e-13       # below this the comparison would measure the last bits of the square root
MIN_REL_FERR = 0.05      # ferr / ||data|| of every case: the identity's cancellation stays out of the comparison


def draw_seed(name):
    return 100 + SPARSE_CASES[name][4]


def matrix(name):
    """The case's data as a canonical float32 csr_matrix."""
    m, n, _, density, seed = SPARSE_CASES[name]
    rng = np.random.RandomState(seed)
    A = sp.random(m, n, density=density, random_state=rng, data_rvs=lambda k: 0.25 + rng.rand(k), dtype=np.float64).tolil()
    A[m // 3, :] = 0.25 + rng.rand(n)
    A[:, n // 3] = (0.25 + rng.rand(m)).reshape(m, 1)
    for r in (m // 2, m - 1):
        A[r, :] = 0.0
    for c in (n // 2, 0):
        A[:, c] = 0.0
    A = A.tocsr().astype(np.float32)
    A.eliminate_zeros()
    A.sum_duplicates()
    return A


def identity_ferr(d64, C, U, R):
    """The trace identity of the module docstring in float64, ||data||^2 as the sum of the row norms."""
    vn = float(np.sum(np.sum(d64 ** 2, axis=1)))
    Mt = np.dot(np.dot(C.T, d64), R.T)
    f2 = vn - 2.0 * float(np.sum(U * Mt)) + float(np.sum(np.dot(np.dot(C.T, C), U) * np.dot(U, np.dot(R, R.T))))
    return float(np.sqrt(max(f2, 0.0)))


_cache = {}


def case(name, kind):
    """dict(sparse csr float32, data dense float32, rrank, seed, rid, cid, rcnt, ccnt, margins, C, U, R, ferr, ferr_twin, gram,
    ferr_dense_twin, kappa_c, kappa_r, tol_U, norm): the float64 oracle of one factorize() on toarray()."""
    if (name, kind) not in _cache:
        A = matrix(name)
        d = A.toarray()
        d64 = d.astype(np.float64)
        rrank, seed = SPARSE_CASES[name][2], draw_seed(name)
        margins = []
        rid, cid, rcnt, ccnt = co.draw(d64, rrank, seed, cmd=(kind == "cmd"), margins=margins)
        C, U, R = co.compute_ucr(d64, rid, rcnt, cid, ccnt)
        gram = co.gram_form(d64, rid, rcnt, cid, ccnt)
        kc, kr = cc.cond(gram["kept_c"]), cc.cond(gram["kept_r"])
        _cache[(name, kind)] = dict(sparse=A, data=d, rrank=rrank, seed=seed, rid=rid, cid=cid, rcnt=rcnt, ccnt=ccnt, margins=margins,
                                    C=C, U=U, R=R, ferr=co.ferr(d64, C, U, R), ferr_twin=identity_ferr(d64, C, U, R), gram=gram,
                                    ferr_dense_twin=co.twin(d64, rid, rcnt, cid, ccnt)["ferr"],
                                    kappa_c=kc, kappa_r=kr, tol_U=(kc + kr) * cc.JACOBI_RTOL, norm=float(np.linalg.norm(d64)))
    return _cache[(name, kind)]


def twin_deviation(c):
    """|identity - direct| of the oracle's error, relative to ||data||."""
    return abs(c["ferr_twin"] - c["ferr"]) / c["norm"]


def measure():
    """Per case and kind: kappa_c, kappa_r, tol_U, the identity's deviation, ferr / ||data|| and the deviation of the dense path's
    float32 twin."""
    out = {}
    for name in SPARSE_CASES:
        for kind in KINDS:
            c = case(name, kind)
            out["%s_%s" % (kind, name)] = dict(kappa_c=c["kappa_c"], kappa_r=c["kappa_r"], tol_U=c["tol_U"], ferr=twin_deviation(c),
                                               ferr_rel=c["ferr"] / c["norm"], ferr_dense=abs(c["ferr_dense_twin"] - c["ferr"]) / c["norm"])
    return out


def tolerances():
    """The committed figures (tests/golden/cur_sparse_tolerances.json, written by tests/golden/gen_golden_cur_sparse.py)."""
    with open(TOL_PATH) as f:
        return json.load(f)


def device_tol_ferr():
    """FACTOR x the largest identity-vs-direct deviation over all cases, floored at FERR_FLOOR."""
    return max(cc.FACTOR * tolerances()["ferr_max"], FERR_FLOOR)


def device_tol_ferr_dense():
    """What the sparse and the dense device run may differ by: FACTOR x the largest deviation of the dense path's float32 twin from
    the oracle on these data, plus the sparse run's own tolerance."""
    return cc.FACTOR * tolerances()["ferr_dense_max"] + device_tol_ferr()
