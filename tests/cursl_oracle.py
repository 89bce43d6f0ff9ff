"""Float64 NumPy restatement of pymf/cursl.py (dense data): the leverage-score probabilities and the draws.

`comp_prob` (cursl.py:66-85) takes the full dense SVD of its argument -- the `k` it hands to SVD is ignored for dense data --
and svd.py keeps the triples whose eigenvalue of the Gram matrix is > 1e-8, in descending order; `V[:k]` is therefore the
leading kk = min(k, rank) right singular vectors.  Here they come from numpy.linalg.svd with the same cut on s^2.  The draws
(cur.py:69-82), CMD's merge (cmd.py:56-70), computeUCR and its device twin are those of tests/cur_oracle.py.
tests/test_cursl_oracle_golden.py holds this file to goldens made by the real reference.
"""
import numpy as np

import cur_oracle as co

EPS = 1e-8            # svd.py:74, on the eigenvalues of the Gram matrix


def leverage(d, k):
    """(the unnormalised leverage of every column of d: sum of squares over the leading kk right singular vectors; kk;
    the eigenvalues s^2 of the Gram matrix, descending, all of them)."""
    d = np.asarray(d, dtype=np.float64)
    _, s, Vt = np.linalg.svd(d, full_matrices=False)
    lam = s ** 2
    V = Vt[lam > EPS]
    A = V[:k, :] ** 2.0
    return A.sum(axis=0), int(A.shape[0]), lam


def comp_prob(d, k):                                           # cursl.py:66-85
    lev, _, _ = leverage(d, k)
    p = lev / k
    p /= np.sum(p)
    return p


def sample_probability(data, rrank, crank):                    # cursl.py:87-91
    data = np.asarray(data, dtype=np.float64)
    pcol = comp_prob(data, rrank)
    prow = comp_prob(data.T, crank)
    return prow.reshape(-1, 1), pcol.reshape(-1, 1)


def ranks(data, rrank):
    """(_rrank, _crank) as CURSL.__init__ leaves them: crank follows rrank (cursl.py:63), 0 = all."""
    rows, cols = np.asarray(data).shape
    return (rrank, rrank) if rrank > 0 else (rows, cols)


def draw(data, rrank, seed, margins=None):
    """(rid, cid, rcnt, ccnt, prow, pcol) of CURSL.factorize() under np.random.seed(seed): cmd.py:72-89 with the
    probabilities above; rows first, then columns.  margins: as cur_oracle.sample."""
    nr, nc = ranks(data, rrank)
    np.random.seed(seed)
    prow, pcol = sample_probability(data, nr, nc)
    rid = co.sample(nr, prow, margins)
    cid = co.sample(nc, pcol, margins)
    rid, cid, rcnt, ccnt = co.cmdinit(rid, cid)
    return rid, cid, rcnt, ccnt, prow, pcol


def gap_factor(lam, kk):
    """1 + lambda_kk / (lambda_kk - lambda_kk+1): how far a relative error of the eigen-solver moves the projector onto the
    leading kk eigenvectors; 1 when the kk vectors are all there are (lam: every eigenvalue, descending; those <= EPS are cut)."""
    rank = int(np.sum(lam > EPS))
    if kk >= rank:
        return 1.0
    return 1.0 + lam[kk - 1] / (lam[kk - 1] - lam[kk])
