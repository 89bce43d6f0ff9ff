"""The sparse-form distances of k_sivm_csc_pass (pymf_amd/csrc/pmf_sivm_csc.h) restated in float32 NumPy, and the two selection
rules on top of any distance function -- the float32 twin that tests/test_sivm_sparse_cases.py holds against the float64 oracle
on toarray() (sivm_oracle.update_w, colsel_oracle.laesa_update_w).

  distance32   per column, over its stored entries (v, r) only, every operation in float32:
                 l2      sqrt(max(|x|^2 + sum [(v - x_r)^2 - x_r^2], 0))
                 l1      max(|x|_1 + sum [|v - x_r| - |x_r|], 0)
                 cosine  1 - sum v x_r / (sqrt(sum v^2) |x| + 1e-9)
               a column measured against itself: exactly 0 under l2 and l1; an empty column is the origin; idx = -1 measures
               against the origin.  The sums run in entry order (the device sums a column in TEAM interleaved strands: another
               order of the same float32 terms).
  select       SIVM's recurrence (sivm.py:145-201) or LAESA's running minimum (laesa.py:63-82) in float64 on such distances
"""
import numpy as np

EPS = 10 ** -8          # sivm.py:170
f4 = np.float32


def distance32(csc, idx, metric):
    m, n = csc.shape
    indptr, rows, v = csc.indptr, csc.indices, csc.data.astype(f4)
    x = np.zeros(m, dtype=f4)
    xx, x1 = f4(0), f4(0)
    if idx >= 0:
        lo, hi = indptr[idx], indptr[idx + 1]
        x[rows[lo:hi]] = v[lo:hi]
        for e in range(lo, hi):
            xx = f4(xx + v[e] * v[e])
            x1 = f4(x1 + abs(v[e]))
    col = np.repeat(np.arange(n), np.diff(indptr))
    xr = x[rows]
    s = np.zeros(n, dtype=f4)
    if metric == "l2":
        d = v - xr
        np.add.at(s, col, d * d - xr * xr)
        out = np.sqrt(np.maximum(xx + s, f4(0)))
    elif metric == "l1":
        np.add.at(s, col, np.abs(v - xr) - np.abs(xr))
        out = np.maximum(x1 + s, f4(0))
    elif metric == "cosine":
        nn = np.zeros(n, dtype=f4)
        np.add.at(s, col, v * xr)
        np.add.at(nn, col, v * v)
        out = f4(1) - s / (np.sqrt(nn) * np.sqrt(xx) + f4(1e-9))
    else:
        raise ValueError(metric)
    assert out.dtype == f4
    if idx >= 0 and metric != "cosine":
        out[idx] = 0
    return out.astype(np.float64)


def _argmax(s):
    """the lowest index of the largest score; a NaN score never wins (sivm_better, pmf_colsweep.h)"""
    return int(np.argmax(np.where(np.isnan(s), -np.inf, s)))


def select(dist, n, k, init="fastmap", rule="sivm", scores=None):
    """`select` of update_w under `rule` ('sivm', 'laesa') with dist(idx) -> the n distances to column idx (-1: the origin)."""
    if init == "fastmap":
        cur = 0
        for _ in range(3):
            d = dist(cur)
            cur = _argmax(d)
        if scores is not None:
            scores.append(d.copy())
    elif init == "origin":
        cur = -1
        d = dist(cur)
    else:
        raise ValueError(init)
    sel = [cur]
    if rule == "laesa":
        dmin = dist(sel[-1])
        for _ in range(k - 1):
            d = dist(sel[-1])
            dmin = np.where(d < dmin, d, dmin)
            if scores is not None:
                scores.append(dmin.copy())
            sel.append(_argmax(dmin))
        return sel
    a = np.log(np.max(d))
    d_square, d_sum, d_ij = np.zeros(n), np.zeros(n), np.zeros(n)
    for l in range(1, k):
        with np.errstate(invalid="ignore"):               # (a float32 cosine distance of a column to itself may be -6e-8)
            d = np.log(dist(sel[l - 1]) + EPS)
        d_ij += d * d_sum
        d_sum += d
        d_square += d ** 2
        it = d_ij + a * d_sum - (l / 2.0) * d_square
        if scores is not None:
            scores.append(it.copy())
        sel.append(_argmax(it))
    return sel


def select32(csc, k, metric="l2", init="fastmap", rule="sivm"):
    return select(lambda idx: distance32(csc, idx, metric), csc.shape[1], k, init, rule)
