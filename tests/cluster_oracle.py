"""NumPy restatement of pymf.Kmeans (pymf/kmeans.py) and pymf.Cmeans (pymf/cmeans.py) under NMF.factorize (nmf.py:171-202)
-- float64 test oracle.  The random draw of kmeans.py:69 is an argument (`sel`), so the oracle itself is deterministic."""
import numpy as np

from cnmf_oracle import _converged

EPS = 10 ** -8          # nmf.py:69
FUZZ = 1.75             # cmeans.py:73


def blobs(m, n, nb, seed, sigma=0.1, spread=0.02):
    """Planted clusters: centres C = U[0,1)^(m x nb), V = C[:, labels] + sigma randn (rounded to float32),
    W0 = C + spread randn: the true centres, perturbed.  Returns (V, W0, labels)."""
    rs = np.random.RandomState(seed)
    C = rs.random_sample((m, nb))
    labels = rs.randint(0, nb, size=n)
    V = (C[:, labels] + sigma * rs.randn(m, n)).astype(np.float32)
    W0 = C + spread * rs.randn(m, nb)
    return V, W0, labels


def pdist(W, data):
    """dist.pdist(W, data, 'l2') (dist.py:57-63,107-124): d[j, c] = ||data[:, c] - W[:, j]||."""
    d = np.empty((W.shape[1], data.shape[1]))
    for j in range(W.shape[1]):
        d[j] = np.sqrt(((data - W[:, j:j + 1]) ** 2).sum(axis=0))
    return d


def frobenius(data, W, H):
    return np.sqrt(np.sum((data - np.dot(W, H)) ** 2))                # nmf.py:100-114


def kmeans_update_h(data, W):
    """kmeans.py:75-79 -> (assigned, H, smallest (d2 - d1) / ||v|| over the samples)."""
    d = pdist(W, data)
    assigned = np.argmin(d, axis=0)
    H = np.zeros((W.shape[1], data.shape[1]))
    H[assigned, np.arange(data.shape[1])] = 1.0
    gap = np.inf
    if d.shape[0] > 1:
        s = np.sort(d, axis=0)
        vn = np.sqrt((data ** 2).sum(axis=0))
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = float(np.where(vn > 0, (s[1] - s[0]) / vn, np.inf).min())
    return assigned, H, gap


def kmeans_update_w(data, W, assigned):
    """kmeans.py:82-87, on a copy of W."""
    W = W.copy()
    for i in range(W.shape[1]):
        idx = np.where(assigned == i)[0]
        if len(idx) > 1:
            W[:, i] = np.sum(data[:, idx], axis=1) / len(idx)
    return W


def cmeans_update_h(data, W):
    """cmeans.py:71-81."""
    k = W.shape[1]
    d = pdist(W, data) + EPS
    H = np.zeros((k, data.shape[1]))
    for i in range(k):
        for j in range(k):
            H[i, :] += (d[i, :] / d[j, :]) ** (2.0 / (FUZZ - 1))
    return np.where(H > 0, 1.0 / H, 0)


def cmeans_update_w(data, W, H):
    """cmeans.py:83-86, on a copy of W."""
    W = W.copy()
    for i in range(W.shape[1]):
        W[:, i] = (H[i:i + 1, :] * data).sum(axis=1) / (H[i, :].sum() + EPS)
    return W


def _loop(data, W, H, state, step_w, step_h, niter, compute_w, compute_h, compute_err):
    n = data.shape[1]
    ferr = np.zeros(niter)
    for i in range(niter):                                            # nmf.py:182-202
        if compute_w:
            W = step_w(W, H, state)
        if compute_h:
            H = step_h(W, state)
        if compute_err:
            ferr[i] = frobenius(data, W, H)
            if i > 1 and _converged(ferr, i, n):
                ferr = ferr[:i]
                break
    return W, H, ferr


def kmeans(data, k, sel=None, W=None, niter=1, compute_w=True, compute_h=True, compute_err=True):
    """Kmeans(data, k).factorize(niter, ...) from the centres data[:, sorted(sel)], or from W.
    Returns (W, H, assigned, ferr, smallest gap (d2 - d1) / ||v|| over the whole run)."""
    data = np.asarray(data, dtype=np.float64)
    W = data[:, np.sort(np.asarray(sel))].copy() if W is None else np.array(W, dtype=np.float64)
    st = {"gap": np.inf}

    def step_h(W, st):
        st["assigned"], H, g = kmeans_update_h(data, W)
        st["gap"] = min(st["gap"], g)
        return H

    H = step_h(W, st)                                                 # init_h, kmeans.py:62-65
    W, H, ferr = _loop(data, W, H, st, lambda W, H, st: kmeans_update_w(data, W, st["assigned"]), step_h,
                       niter, compute_w, compute_h, compute_err)
    return W, H, st["assigned"], ferr, st["gap"]


def cmeans(data, W, H, niter=1, compute_w=True, compute_h=True, compute_err=True):
    """Cmeans.factorize(niter, ...) from (W, H).  Returns (W, H, ferr)."""
    data = np.asarray(data, dtype=np.float64)
    return _loop(data, np.array(W, dtype=np.float64), np.array(H, dtype=np.float64), None,
                 lambda W, H, st: cmeans_update_w(data, W, H), lambda W, st: cmeans_update_h(data, W),
                 niter, compute_w, compute_h, compute_err)
