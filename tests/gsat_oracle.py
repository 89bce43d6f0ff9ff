"""Float64 NumPy restatement of SIVM_GSAT's init_w, online_update_w and update_w (reference pymf/sivm_gsat.py:78-125 with
vol.py:24-34 and dist.py:32-35,57-63,107-124) for the tests, with a list for `select`: the twin for sequences that the goldens
do not cover (vectors that are no data columns, a start from another selection).

  Walk(V, k, measure, W=None, select=None)   the state: W (a copy), select, and from the first probe on D, V and _v
  .online_update_w(vec)                      -> (True, s) or (False, -1), exactly as the reference decides
  .update_w(n)                               the probe of data column n behind its `n not in select` test; the slot, -1 or -2
  walk(V, k, idx, measure, ...)              all of idx in order -> dict(slots, select, W, v, V, margin)
reference_f1=True takes vol.py's factor f1 with the reference's float32 roundings (f1 below): what the goldens hold to 1e-12.
The default is the exact factor, which the device folds into its pivots; the decisions are the same, f1 being common to all
volumes of a probe (while it is not 0: the reference's is from 20 bases on).
The decision margin of a probe is |max_i v[i] - V| / V: how far a rounding error would have to move a volume to flip it.
"""
import math

import numpy as np


def f1(j, reference=False):
    """vol.py:30-31.  The reference takes j as a float32, and the factorial (a gamma function) of a float32, its square and
    the product with 2^j stay float32: its f1 carries float32 roundings (up to 9e-08 relative at 2 .. 19 bases) and is 0
    from 20 bases on, where the denominator overflows.  reference=False: the exact factor in float64."""
    if reference:
        import scipy.special
        j = np.float32(j)
        with np.errstate(over="ignore", under="ignore"):
            return float((-1.0) ** (j + 1) / ((2 ** j) * (scipy.special.factorial(j)) ** 2))
    return (-1.0) ** (j + 1) / ((2.0 ** j) * float(math.factorial(j)) ** 2)


def cmdet(d, reference_f1=False):
    """vol.py:24-34: the Cayley-Menger volume from a matrix of (not squared) distances"""
    n = d.shape[0]
    D = np.ones((n + 1, n + 1))
    D[0, 0] = 0.0
    D[1:, 1:] = d ** 2
    return float(np.sqrt(np.abs(f1(n - 1, reference_f1) * np.linalg.det(D))))


def l2_distance(d, vec):
    return np.sqrt(((d - vec) ** 2).sum(axis=0)).reshape(-1)


def l1_distance(d, vec):
    return np.sum(np.abs(d - vec), axis=0).reshape(-1)


def pdist(W):
    """dist.py:107-124 for A = B = W, l2"""
    k = W.shape[1]
    d = np.zeros((k, k))
    for a in range(k):
        d[a, :] = l2_distance(W, W[:, a:a + 1])
    return d


class Walk(object):
    def __init__(self, V, k, measure="l2", W=None, select=None, reference_f1=False):
        self.reference_f1 = reference_f1
        self.data = np.asarray(V, dtype=np.float64)
        self.k = int(k)
        self.distfunc = {"l2": l2_distance, "l1": l1_distance}[measure]
        self.select = list(range(self.k)) if select is None else [int(s) for s in select]          # sivm_gsat.py:78-80
        self.W = np.array(self.data[:, self.select] if W is None else W, dtype=np.float64)
        self.margin = np.inf

    def online_update_w(self, vec):                            # sivm_gsat.py:82-117
        k = self.k
        vec = np.asarray(vec, dtype=np.float64).reshape(-1)
        if not hasattr(self, "D"):
            self.D = np.zeros((k + 1, k + 1))
            self.D[:k, :k] = pdist(self.W)
            self.V = cmdet(self.D[:k, :k], self.reference_f1)
        tmp = self.distfunc(self.W, vec.reshape(-1, 1))
        self.D[k, :-1] = tmp
        self.D[:-1, k] = tmp
        v = np.zeros(k + 1)
        for i in range(k):
            s = np.setdiff1d(np.arange(k + 1), [i])
            v[i] = cmdet(self.D[s, :][:, s], self.reference_f1)
        v[-1] = self.V
        if self.V > 0:
            self.margin = min(self.margin, abs(v[:k].max() - self.V) / self.V)
        s = int(np.argmax(v))
        if s < k:
            self.W[:, s] = vec
            self.D[:k, :k] = pdist(self.W)
            if not hasattr(self, "_v"):
                self._v = [self.V]
            self.V = float(v[s])
            self._v.append(float(v[s]))
            return True, s
        return False, -1

    def update_w(self, n):                                     # sivm_gsat.py:119-125 with the index given
        n = int(n)
        if n in self.select:
            return -2
        updated, s = self.online_update_w(self.data[:, n])
        if updated:
            self.select[s] = n
        return s


def walk(V, k, idx, measure="l2", W=None, select=None, reference_f1=False):
    w = Walk(V, k, measure, W=W, select=select, reference_f1=reference_f1)
    slots = [w.update_w(n) for n in idx]
    return dict(slots=np.array(slots, dtype=np.int64), select=list(w.select), W=w.W, v=list(getattr(w, "_v", [])),
                V=getattr(w, "V", None), margin=float(w.margin), D=getattr(w, "D", None))


def draws(seed, niter, n):
    """The indices that `niter` calls of update_w draw behind np.random.seed(seed) (sivm_gsat.py:120)"""
    rs = np.random.RandomState(seed)
    return np.floor(rs.random_sample(niter) * n).astype(np.int64)
