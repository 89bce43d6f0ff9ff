"""Float64 NumPy restatement of SIVM (reference pymf/sivm.py, pymf/aa.py) for the tests.

  update_w      SIVM.update_w (sivm.py:145-201): the distance passes, the recurrence, the argmax chain; optionally with every
                distance rounded to float32 (what the device's fp32 distance sums amount to) and with the scores of every
                step handed back (the argmax gap of tests/test_sivm_cases.py)
  simplex_qp    the EXACT minimiser of  1/2 x^T S x - f^T x,  x >= 0, sum x = 1  by a primal active-set method: the KKT point
                that cvxopt's interior-point solver approximates (aa.py:93-111)
  update_h      AA.update_h for all columns, with switches for float32 rounding of V, W, the right-hand sides and X
  simplex_rounds  the multiplier search of the device's H step, restated: rounds until |sum x - 1| <= tol
  kkt_violation   how far an H is from the KKT conditions of its columns' problems
"""
import numpy as np

EPS = 10 ** -8          # sivm.py:170


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def distance(V, idx, metric):
    """dist.py:32-35, 57-63, 73-82 (the cosine distance as its formula reads for one vector) against column idx; -1: the origin."""
    x = V[:, idx] if idx >= 0 else np.zeros(V.shape[0])
    if metric == "l2":
        return np.sqrt(((V - x[:, None]) ** 2).sum(axis=0))
    if metric == "l1":
        return np.abs(V - x[:, None]).sum(axis=0)
    if metric == "cosine":
        return 1.0 - V.T.dot(x) / (np.sqrt((V ** 2).sum(axis=0)) * np.sqrt((x ** 2).sum()) + 10 ** -9)
    raise ValueError(metric)


def update_w(V, k, metric="l2", init="fastmap", f32_dist=False, scores=None):
    """(select, W).  scores (a list): receives the score vector of every argmax that appends to select."""
    V = np.asarray(V, dtype=np.float64)
    n = V.shape[1]

    def dist(idx):
        d = distance(V, idx, metric)
        return f32(d) if f32_dist else d

    select = []
    if init == "fastmap":
        cur = 0
        for _ in range(3):
            d = dist(cur)
            cur = int(np.argmax(d))
        if scores is not None:
            scores.append(d.copy())
    elif init == "origin":
        cur = -1
        d = dist(cur)
    else:
        raise ValueError(init)
    maxd = np.max(d)
    select.append(cur)
    d_square, d_sum, d_ij = np.zeros(n), np.zeros(n), np.zeros(n)
    a = np.log(maxd)
    for l in range(1, k):
        d = np.log(dist(select[l - 1]) + EPS)
        d_ij += d * d_sum
        d_sum += d
        d_square += d ** 2
        it = d_ij + a * d_sum - (l / 2.0) * d_square
        if scores is not None:
            scores.append(it.copy())
        select.append(int(np.argmax(it)))
    return select, V[:, select]                 # (a -1 entry is a Python index: the last column, sivm.py:198)


def _active_set(S, f, simplex, x0=None):
    """min 1/2 x^T S x - f^T x over x >= 0 (and sum x = 1 when simplex), S positive definite: primal active set from the
    feasible x0 (default: the barycentre / zero).  Returns (x, multiplier of the sum constraint or 0)."""
    k = len(f)
    if x0 is None:
        x = np.full(k, 1.0 / k) if simplex else np.zeros(k)
    else:
        x = np.array(x0, dtype=np.float64)
    P = x > 0
    lam = 0.0
    for _ in range(20 * k + 20):
        idx = np.flatnonzero(P)
        p = len(idx)
        z = np.zeros(k)
        if p:
            if simplex:
                K = np.zeros((p + 1, p + 1))
                K[:p, :p] = S[np.ix_(idx, idx)]
                K[:p, p] = -1.0
                K[p, :p] = 1.0
                sol = np.linalg.solve(K, np.concatenate([f[idx], [1.0]]))
                z[idx], lam = sol[:p], sol[p]
            else:
                z[idx] = np.linalg.solve(S[np.ix_(idx, idx)], f[idx])
        if p and np.all(z[idx] > 0):
            x = z
            w = f + lam - S.dot(x)               # the negative reduced gradient: <= 0 off the support at the minimiser
            w[P] = -np.inf
            j = int(np.argmax(w))
            if w[j] <= 1e-13 * max(1.0, np.abs(f).max()):
                return x, lam
            P[j] = True
            continue
        if not p:                                # (x = 0, non-negative problem only)
            w = f - S.dot(x)
            j = int(np.argmax(w))
            if w[j] <= 0:
                return x, 0.0
            P[j] = True
            continue
        blocking = idx[z[idx] <= 0]
        alpha = np.min(x[blocking] / (x[blocking] - z[blocking]))
        x = x + alpha * (z - x)
        drop = idx[(z[idx] <= 0) & (x[idx] <= 1e-15 * max(1.0, x.max()))]
        if len(drop) == 0:
            drop = blocking[np.argmin(x[blocking])][None]
        x[drop] = 0.0
        P[drop] = False
    raise RuntimeError("active set did not terminate")


def simplex_qp(S, f):
    return _active_set(np.asarray(S, dtype=np.float64), np.asarray(f, dtype=np.float64), True)[0]


def nnqp(S, f, x0=None):
    return _active_set(np.asarray(S, dtype=np.float64), np.asarray(f, dtype=np.float64), False, x0)[0]


def products(V, W, f32_v=False, f32_w=False, f32_rhs=False):
    Vr = f32(V) if f32_v else np.asarray(V, dtype=np.float64)
    Wr = f32(W) if f32_w else np.asarray(W, dtype=np.float64)
    S = Wr.T.dot(Wr)
    F = Wr.T.dot(Vr)
    return Vr, Wr, S, (f32(F) if f32_rhs else F)


def update_h(V, W, f32_v=False, f32_w=False, f32_rhs=False, f32_x=False):
    """(H, ferr): AA.update_h (aa.py:93-111) with the exact solver, and ||V - W H|| of the operands as used."""
    Vr, Wr, S, F = products(V, W, f32_v, f32_w, f32_rhs)
    H = np.stack([simplex_qp(S, F[:, c]) for c in range(F.shape[1])], axis=1)
    if f32_x:
        H = f32(H)
    return H, float(np.sqrt(((Vr - Wr.dot(H)) ** 2).sum()))


def simplex_rounds(S, F, tol=1e-6, cap=200, f32_rhs=True, f32_x=True):
    """The device's multiplier search per column: lambda = -max f gives x = 0; first multiplier that of the problem without
    the signs; no upper end yet: grow; else Illinois.  Returns (H, rounds per column)."""
    S = np.asarray(S, dtype=np.float64)
    k, n = F.shape
    u = np.linalg.solve(S, np.ones(k))
    H = np.zeros((k, n))
    rounds = np.zeros(n, dtype=np.int64)
    for c in range(n):
        f = F[:, c]
        lam_min = -f.max()
        lam = (1.0 - u.dot(f)) / u.sum()
        if not (u.sum() > 0 and lam > lam_min):
            lam = lam_min + S[np.argmax(f), np.argmax(f)]
        lo, glo, hi, ghi, side = lam_min, -1.0, lam_min, 0.0, 0
        x = np.zeros(k)
        for r in range(1, cap + 1):
            rhs = f + lam
            x = nnqp(S, f32(rhs) if f32_rhs else rhs, x0=x)
            if f32_x:
                x = f32(x)
            g = x.sum() - 1.0
            if abs(g) <= tol:
                break
            if g < 0:
                lo, glo = lam, g
                if side < 0:
                    ghi *= 0.5
                if side != 0:
                    side = -1
            else:
                hi, ghi = lam, g
                if side > 0:
                    glo *= 0.5
                side = 1
            if side == 0:
                lam = lam + 2.0 * (lam - lam_min)
            else:
                nl = (lo * ghi - hi * glo) / (ghi - glo)
                lam = nl if lo < nl < hi else 0.5 * (lo + hi)
        H[:, c] = x
        rounds[c] = r
    return H, rounds


def kkt_violation(S, F, H):
    """(min x, max |sum x - 1|, worst spread of the reduced gradient on the support, worst shortfall off it), the last two
    relative to the largest |f| of the column."""
    G = S.dot(H) - F
    worst_on, worst_off = 0.0, 0.0
    for c in range(H.shape[1]):
        sup = H[:, c] > 0
        scale = max(1.0, np.abs(F[:, c]).max())
        g = G[:, c]
        worst_on = max(worst_on, (g[sup].max() - g[sup].min()) / scale)
        if (~sup).any():
            worst_off = max(worst_off, (g[sup].max() - g[~sup].min()) / scale)
    return float(H.min()), float(np.abs(H.sum(axis=0) - 1.0).max()), worst_on, worst_off
