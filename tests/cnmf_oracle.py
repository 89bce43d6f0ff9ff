"""NumPy restatement of pymf.CNMF (reference pymf/cnmf.py) and of the k-means it initialises from (pymf/kmeans.py,
pymf/dist.py:vq) -- float64 test oracle.  The random draw of kmeans.py:71 is an argument here (`sel`), so the oracle itself
is deterministic; pymf_amd.CNMF draws it with the reference's call."""
import numpy as np

EPS = 10 ** -8          # nmf.py:69
EPS_DEN = 10 ** -9      # cnmf.py:165-166,172


def _pos(m):
    return (np.abs(m) + m) / 2.0          # cnmf.py:139-140


def _neg(m):
    return (np.abs(m) - m) / 2.0          # cnmf.py:142-143


def _converged(ferr, i, n):
    return np.abs(ferr[i] - ferr[i - 1]) / n < EPS      # nmf.py:134-139


def vq(C, X):
    """dist.vq (dist.py:126-130): the index of the nearest centre (column of C) for every column of X; the lowest index
    among equal distances (np.argmin).  Also returns the (d2 - d1) / d2 gap between the best and the second best centre."""
    d = np.empty((C.shape[1], X.shape[1]))
    for j in range(C.shape[1]):                                      # dist.py:108-111 (l2_distance, dist.py:57-63)
        d[j] = np.sqrt(((X - C[:, j:j + 1]) ** 2).sum(axis=0))
    assigned = np.argmin(d, axis=0)
    if d.shape[0] > 1:
        s = np.sort(d, axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = np.where(s[1] > 0, (s[1] - s[0]) / s[1], 1.0)
        gap = float(gap.min())
    else:
        gap = 1.0
    return assigned, gap


def vq_gram(C, X):
    """vq through ||x||^2 - 2 x^T c + ||c||^2 (the form of dist.py:65-71): the same argmin wherever the distances are
    not near-tied, at the cost of one product -- for large planted-cluster data."""
    d = (X * X).sum(axis=0)[None, :] - 2.0 * np.dot(C.T, X) + (C * C).sum(axis=0)[:, None]
    return np.argmin(d, axis=0), 1.0


def kmeans(data, k, sel, niter=10, vq_fn=vq):
    """Kmeans(data, k).factorize(niter) under NMF.factorize (nmf.py:171-202, kmeans.py:64-87) from the centres data[:, sel].
    Returns (assigned, ferr, smallest relative distance gap seen)."""
    data = np.asarray(data, dtype=np.float64)
    n = data.shape[1]
    W = data[:, np.sort(np.asarray(sel))].copy()                     # kmeans.py:71-74
    assigned, gap = vq_fn(W, data)                                   # init_h -> update_h, kmeans.py:64-67,76-81
    ferr = np.zeros(niter)                                           # nmf.py:179-180
    for i in range(niter):
        for j in range(k):                                           # update_w, kmeans.py:83-87
            idx = np.where(assigned == j)[0]
            if len(idx) > 1:
                W[:, j] = np.sum(data[:, idx], axis=1) / len(idx)
        assigned, g = vq_fn(W, data)                                 # update_h
        gap = min(gap, g)
        H = np.zeros((k, n))
        H[assigned, np.arange(n)] = 1.0
        ferr[i] = np.sqrt(np.sum((data - np.dot(W, H)) ** 2))       # nmf.py:100-114
        if i > 1 and _converged(ferr, i, n):                        # nmf.py:198-202
            ferr = ferr[:i]
            break
    return assigned, ferr, gap


def cnmf_init(data, k, sel, G=None, km_niter=10, vq_fn=vq):
    """CNMF.init_h (cnmf.py:78-103): H from the k-means assignment, G unless given; returns (H, G, assigned)."""
    n = data.shape[1]
    assigned, _, _ = kmeans(data, k, sel, km_niter, vq_fn)                # cnmf.py:84-86
    num_i = np.array([np.sum(assigned == j) for j in range(k)], dtype=np.float64)   # cnmf.py:88-90
    H = np.zeros((k, n))
    H.T[np.arange(n), assigned] = 1.0                                # cnmf.py:92
    H += 0.2 * np.ones((k, n))                                       # cnmf.py:93
    if G is None:                                                    # cnmf.py:95-100
        G = np.zeros((n, k))
        G[np.arange(n), assigned] = 1.0
        G += 0.01
        G /= np.tile(np.reshape(num_i[assigned], (-1, 1)), G.shape[1])
    return H, G, assigned


def cnmf_factorize(data, H, G, W=None, niter=10, compute_w=True, compute_h=True, compute_err=True, gram=None, w_round=None):
    """CNMF.factorize (cnmf.py:108-187) from (H, G, W); W None: data G.  Returns (W, H, G, ferr).
    gram: a matrix to stand in for data^T data; w_round: applied to W = data G wherever it is formed (both for
    tests/cnmf_cases.py: what a float32 C and a float32 W cost whatever the arithmetic)."""
    w_round = w_round or (lambda w: w)
    data = np.asarray(data, dtype=np.float64)
    H = np.array(H, dtype=np.float64)
    G = np.array(G, dtype=np.float64)
    W = w_round(np.dot(data, G)) if W is None else np.array(W, dtype=np.float64)   # cnmf.py:102-103
    n = data.shape[1]
    XtX = np.dot(data.T, data) if gram is None else np.asarray(gram, dtype=np.float64)   # cnmf.py:150
    XtX_pos, XtX_neg = _pos(XtX), _neg(XtX)                          # cnmf.py:151-152
    ferr = np.zeros(niter)                                           # cnmf.py:154
    for i in range(niter):
        A = np.dot(XtX_neg, G)                                       # cnmf.py:159
        B = np.dot(XtX_pos, G)                                       # cnmf.py:160
        if compute_h:                                                # cnmf.py:162-167
            HGt = np.dot(H.T, G.T)
            ha = B + np.dot(HGt, A)
            hb = A + np.dot(HGt, B) + EPS_DEN
            H = (H.T * np.sqrt(ha / hb)).T
        if compute_w:                                                # cnmf.py:169-175
            S = np.dot(H, H.T)
            wa = np.dot(XtX_pos, H.T) + np.dot(A, S)
            wb = np.dot(XtX_neg, H.T) + np.dot(B, S) + EPS_DEN
            G = G * np.sqrt(wa / wb)
            W = w_round(np.dot(data, G))
        if compute_err:                                              # cnmf.py:177-179, frobenius_norm nmf.py:100-114
            ferr[i] = np.sqrt(np.sum((data - np.dot(W, H)) ** 2))
        if i > 1 and compute_err and _converged(ferr, i, n):        # cnmf.py:184-187
            ferr = ferr[:i]
            break
    return W, H, G, ferr
