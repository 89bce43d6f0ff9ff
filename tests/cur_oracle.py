"""Float64 NumPy restatement of pymf/cur.py and pymf/cmd.py (dense data) with svd.py's pinv, and its "float32 twin".

The oracle is the reference's arithmetic written out: sample_probability (cur.py:84-97), sample (cur.py:69-82), CMD's merge
of repeated indices (cmd.py:56-70), computeUCR (cur.py:99-120) through pinv (svd.py:27-45) on the restated SVD of
tests/svd_oracle.py, and frobenius_norm (svd.py:92-107).  tests/test_cur_oracle_golden.py holds it to goldens made by the
real reference.

The twin models the device path: the data are rounded to float32 (the upload), the middle factor is
(C^T C)^+ (dc o (Cg^T data Rg^T) o dr) (R R^T)^+ with every product in float64 and svd.py's 1e-8 cut on the eigenvalues of
C^T C and R R^T, and for the error C U and R are rounded to float32, multiplied in float32 and subtracted from the float32
data in float32 (the residual pass), the squares summed in float64.  `middle32=True` forms Cg^T data Rg^T in float32
instead: what the float64 MFMA is there to avoid (tests/test_cur_cases.py measures it).
"""
import numpy as np

import svd_oracle as so

EPS = 1e-8            # svd.py:74, the default of pinv


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def sample_probability(data):                                  # cur.py:84-97
    dsquare = np.asarray(data, dtype=np.float64)[:, :] ** 2
    prow = np.array(dsquare.sum(axis=1), np.float64)
    pcol = np.array(dsquare.sum(axis=0), np.float64)
    prow /= prow.sum()
    pcol /= pcol.sum()
    return prow.reshape(-1, 1), pcol.reshape(-1, 1)


def sample(s, probs, margins=None):                            # cur.py:69-82
    """The sorted indices of s draws from NumPy's global stream.  margins (a list): the distance of every draw from the
    nearest entry of the cumulative sum is appended."""
    cum = np.cumsum(probs.flatten())
    ind = np.zeros(s, np.int32)
    for i in range(s):
        v = np.random.rand()
        hit = np.where(cum >= v)[0]
        if hit.shape[0] == 0:
            raise IndexError("a draw exceeds the last cumulative probability")
        ind[i] = hit[0]
        if margins is not None:
            margins.append(float(np.min(np.abs(cum - v))))
    return np.sort(ind)


def cmdinit(rid, cid):                                         # cmd.py:56-70
    nr, rc = np.unique(rid, return_counts=True)
    nc, cc = np.unique(cid, return_counts=True)
    return np.int32(nr), np.int32(nc), rc.astype(np.float64), cc.astype(np.float64)


def draw(data, rrank, seed, cmd=False, margins=None):
    """(rid, cid, rcnt, ccnt) of CUR.factorize() / CMD.factorize() under np.random.seed(seed): rows first, then columns;
    crank follows rrank (cur.py:60), 0 = all."""
    rows, cols = data.shape
    nr = rrank if rrank > 0 else rows
    nc = rrank if rrank > 0 else cols
    np.random.seed(seed)
    prow, pcol = sample_probability(data)
    rid = sample(nr, prow, margins)
    cid = sample(nc, pcol, margins)
    if cmd:
        return cmdinit(rid, cid)
    return rid, cid, np.ones(len(rid)), np.ones(len(cid))


def pinv(A, eps=EPS):                                          # svd.py:27-45
    U, S, V = so.svd(np.asarray(A, dtype=np.float64))
    s = np.diag(S)
    inv = np.where(s > eps, 1.0 / s, 0.0)
    return np.dot(V.T, inv[:, np.newaxis] * U.T)


def factors(data, rid, rcnt, cid, ccnt):
    """C = data[:, cid] diag(sqrt(ccnt)) and R = diag(sqrt(rcnt)) data[rid, :] (cur.py:111-112)."""
    data = np.asarray(data, dtype=np.float64)
    C = np.dot(data[:, cid].reshape((data.shape[0], len(cid))), np.diag(np.asarray(ccnt, dtype=np.float64) ** (1 / 2)))
    R = np.dot(np.diag(np.asarray(rcnt, dtype=np.float64) ** (1 / 2)), data[rid, :].reshape((len(rid), data.shape[1])))
    return C, R


def compute_ucr(data, rid, rcnt, cid, ccnt):                   # cur.py:99-120
    data = np.asarray(data, dtype=np.float64)
    C, R = factors(data, rid, rcnt, cid, ccnt)
    U = np.dot(np.dot(pinv(C), data), pinv(R))
    return C, U, R


def ferr(data, C, U, R):                                       # svd.py:92-107
    return float(np.sqrt(np.sum((np.asarray(data, dtype=np.float64) - np.dot(np.dot(C, U), R)) ** 2)))


def sym_pinv(G, eps=EPS):
    """(pseudo-inverse of the symmetric G over its eigenvalues > eps, kept eigenvalues, dropped eigenvalues)."""
    w, E = np.linalg.eigh(G)
    keep = w > eps
    order = np.argsort(w[keep])[::-1]
    wk, Ek = w[keep][order], E[:, keep][:, order]
    return np.dot(Ek / wk, Ek.T), wk, w[~keep]


def gram_form(data, rid, rcnt, cid, ccnt, middle32=False):
    """dict(U, kept_c, dropped_c, kept_r, dropped_r): the middle factor as the device forms it, from float64 data holding
    float32 values.  middle32: Cg^T data Rg^T is a float32 product of the float32 values."""
    data = np.asarray(data, dtype=np.float64)
    dc, dr = np.sqrt(np.asarray(ccnt, dtype=np.float64)), np.sqrt(np.asarray(rcnt, dtype=np.float64))
    Cg, Rg = data[:, cid], data[rid, :]
    Pc, kc, xc = sym_pinv(np.dot(Cg.T, Cg) * np.outer(dc, dc))
    Pr, kr, xr = sym_pinv(np.dot(Rg, Rg.T) * np.outer(dr, dr))
    if middle32:
        c32, d32, r32 = (np.asarray(a, dtype=np.float32) for a in (Cg, data, Rg))
        M = np.dot(np.dot(c32.T, d32), r32.T).astype(np.float64)
    else:
        M = np.dot(np.dot(Cg.T, data), Rg.T)
    U = np.dot(np.dot(Pc, dc[:, None] * M * dr[None, :]), Pr)
    return dict(U=U, kept_c=kc, dropped_c=xc, kept_r=kr, dropped_r=xr)


def twin(data, rid, rcnt, cid, ccnt):
    """dict(C, U, R, ferr) of the device model described in the module docstring."""
    d32 = f32(data)
    C, R = factors(d32, rid, rcnt, cid, ccnt)
    U = gram_form(d32, rid, rcnt, cid, ccnt)["U"]
    W = np.dot(C, U).astype(np.float32)
    H = R.astype(np.float32)
    resid = d32.astype(np.float32) - np.dot(W, H)
    return dict(C=C, U=U, R=R, ferr=float(np.sqrt(np.sum(resid.astype(np.float64) ** 2))))
