"""Float64 NumPy restatement of SIVM_SGREEDY.update_w (reference pymf/sivm_sgreedy.py:96-133 with vol.py:24-34) for the tests.

  update_w       the literal one: SIVM's start (sivm_oracle.distance), then per round and per candidate the full Cayley-Menger
                 determinant of the sorted selection + candidate from l2 distances (the root taken and squared again, as
                 cmdet does), first index on a tie, the reference's order of `select`, `_v`
  update_w_twin  the device's formulation: squared l2 distances formed and summed in float32, CM_S made of those same values,
                 score = sqrt(|f1 det(CM_S) b^T inv(CM_S) b|) -- what the tolerances of the device comparison are derived from
Both hand back the score vector of every round (scores) and the picks in selection order.
"""
import math

import numpy as np

import sivm_oracle as so

CHUNK = 1 << 15


def f1(j):
    """vol.py:30-31 for a selection + candidate of j + 1 points"""
    return (-1.0) ** (j + 1) / ((2.0 ** j) * float(math.factorial(j)) ** 2)


def start(V, metric, init, f32_dist=False):
    """init_sivm (sivm.py:145-166): select[0]"""
    def dist(idx):
        d = so.distance(V, idx, metric)
        return so.f32(d) if f32_dist else d
    if init == "fastmap":
        cur = 0
        for _ in range(3):
            cur = int(np.argmax(dist(cur)))
        return cur
    if init == "origin":
        return -1
    raise ValueError(init)


def f32_sqdist(V32, idx):
    """the squared l2 distances to column idx formed in float32 throughout: differences, squares and a running sum down the
    rows (one accumulator; the device keeps four, which rounds no worse)"""
    d = V32 - V32[:, idx][:, None]
    s = np.zeros(V32.shape[1], dtype=np.float32)
    for r in range(V32.shape[0]):
        s += d[r] * d[r]
    return s.astype(np.float64)


def reference_order(picks):
    return sorted(picks[:-1]) + picks[-1:]


def update_w(V, k, metric="l2", init="fastmap", scores=None):
    """(select, W, v, picks)"""
    V = np.asarray(V, dtype=np.float64)
    n = V.shape[1]
    next_sel = [start(V, metric, init)]
    picks = list(next_sel)
    v = []
    for _ in range(k - 1):
        next_sel = sorted(next_sel)                                   # sivm_sgreedy.py:108
        S = V[:, next_sel]                                            # (-1 is a Python index: the last column)
        t = len(next_sel)
        D = np.sqrt(((S[:, :, None] - S[:, None, :]) ** 2).sum(axis=0))
        vol = np.empty(n)
        for c0 in range(0, n, CHUNK):
            X = V[:, c0:c0 + CHUNK]
            dt = np.sqrt(((S[:, :, None] - X[:, None, :]) ** 2).sum(axis=0))      # [t][chunk]
            cm = np.ones((X.shape[1], t + 2, t + 2))
            cm[:, 0, 0] = 0.0
            cm[:, 1:t + 1, 1:t + 1] = (D ** 2)[None]
            cm[:, 1:t + 1, t + 1] = (dt ** 2).T
            cm[:, t + 1, 1:t + 1] = (dt ** 2).T
            cm[:, t + 1, t + 1] = 0.0
            vol[c0:c0 + CHUNK] = np.sqrt(np.abs(f1(t) * np.linalg.det(cm)))
        if scores is not None:
            scores.append(vol.copy())
        nxt = int(np.argmax(vol))
        next_sel.append(nxt)
        picks.append(nxt)
        v.append(float(np.max(vol)))
    return list(next_sel), V[:, next_sel], v, picks


def update_w_twin(V, k, metric="l2", init="fastmap", scores=None):
    """(select, W, v, picks) with the device's arithmetic: fp32-rounded squared distances, the Schur form in float64"""
    V = np.asarray(V, dtype=np.float64)
    V32 = V.astype(np.float32)
    n = V.shape[1]
    picks = [start(V, metric, init, f32_dist=True)]
    table = []                                                        # row r: squared distances to pick r, float32-rounded
    v = []
    for t in range(1, k):
        cm = np.ones((t + 1, t + 1))
        cm[0, 0] = 0.0
        for i in range(1, t + 1):
            cm[i, i] = 0.0
            for j in range(i + 1, t + 1):
                cm[i, j] = cm[j, i] = table[i - 1][picks[j - 1]]
        with np.errstate(all="ignore"):
            try:
                M = np.linalg.inv(cm)
            except np.linalg.LinAlgError:
                M = np.full_like(cm, np.nan)
            scale = abs(f1(t) * np.linalg.det(cm))
            table.append(f32_sqdist(V32, picks[-1]))
            B = np.vstack([np.ones(n)] + table)                       # [t + 1][n]
            vol = np.sqrt(np.abs(scale * (B * M.dot(B)).sum(axis=0)))
        if scores is not None:
            scores.append(vol.copy())
        ok = ~np.isnan(vol)
        nxt = int(np.flatnonzero(ok)[np.argmax(vol[ok])]) if ok.any() else 0      # (a NaN never wins on the device)
        picks.append(nxt)
        v.append(float(vol[nxt]))
    select = reference_order(picks)
    return select, V[:, select], v, picks
