"""pymf_amd.SVD -- drop-in for pymf.SVD (reference pymf/svd.py) on MI355X, dense data.

The reference takes the SVD of the data through the eigen-decomposition of the Gram matrix on the short side
(svd.py:110-158): data^T data for rows > cols (`_left_svd`), data data^T otherwise (`_right_svd`); eigenvalues <= 1e-8 are
dropped, the rest sorted descending, S = sqrt, and the other side is projected (U = data V^T S^-1 or V = S^-1 U^T data).
On the device the Gram matrix of the float32 data is formed in float64 on the float64 MFMA (k_prod_f64, the upper block triangle), decomposed by the
float64 Jacobi solver, and the projected side is multiplied in float32.  U (rows x r), S (r x r diagonal)
and V (r x cols) come back as float64 arrays, as the reference returns them; r is the number of eigenvalues kept.

Supported: dense data, one rank, min(rows, cols) <= 2432; scipy.sparse data only as described below.  Without that opt-in
scipy.sparse data raises TypeError; a multi-rank world NotImplementedError (on sparse data ValueError), a larger short side ValueError.  `k` is accepted and ignored for dense data, as in svd.py.

scipy.sparse data (opt-in: `mdl.accept_sparse = True`, the switch NMF and CUR have; SVD and PCA only -- pinv keeps refusing).
The switch is read from the object, not from the class: SVD is also the model inside pinv and the base of the CUR family, and a
value set on the shared class must not make those take sparse data; the class attribute states the default.
The matrix is converted once to canonical CSR (tocsr(), duplicates summed, indices sorted, float32 values) and stays sparse on
the device: the Gram matrix of the short side comes from stored entries in exact fixed point (k_csr_gram), the Jacobi solver is
the dense path's, and the projected side is one pass over the stored entries in float64 (k_csr_proj_f64).  Here
`k` means what it means in the reference's sparse branch (svd.py:165,204): with 0 < k < min(rows, cols) - 1 the leading k
triples above the 1e-8 cut are kept, otherwise all of them.  Deliberate deviations from that branch: U, S, V come back as dense
float64 arrays (the reference returns csc_matrix), and k outside that range keeps every triple where ARPACK's k = min(dim) - 1
silently drops the smallest pair -- the yardstick is the dense path, as for CUR.  frobenius_norm() is evaluated in float64 without
a dense image, ferr^2 = ||data||^2 - 2 <U^T data, S V> + <U^T U, (S V)(S V)^T> (clamped at 0); it needs the factors of the last
factorize(): a rebound U, S or V raises NotImplementedError.  Limits there: min(rows, cols) <= 1024 after padding to 64.

`pinv(A, k=-1, eps=1e-8)` is svd.py:27-45: SVD(A).factorize(), the reciprocals of the singular values above `eps`, then
V^T diag U^T on the host arrays that SVD returns; it has SVD's limits.
"""
import warnings

import numpy as np

from . import _lib
from . import dist as _dist
from .nmf import PrecisionWarning, _is_sparse

__all__ = ["SVD", "pinv"]

MAX_RANK = 2432   # PMF_SVD_MAX_RANK (pmf_svd.h)
MAX_SPARSE_SIDE = 1024   # PMF_GRAM_MAX_NP: the short side of sparse data, padded to 64 (k_csr_gram's slab scheme)


def canonical_csr(data):
    """scipy.sparse `data` as the device takes it: CSR, one entry per position, ascending columns; the caller's matrix is left alone."""
    arr = data.tocsr()
    if not arr.has_canonical_format:
        if arr is data:
            arr = arr.copy()
        arr.sum_duplicates()
    return arr


def check_sparse_limits(name, rows, cols, world_size=1):
    if world_size > 1:
        raise ValueError("%s on scipy.sparse data: one rank only (a multi-rank world is not supported)" % name)
    if -(-min(rows, cols) // 64) * 64 > MAX_SPARSE_SIDE:
        raise ValueError("%s on scipy.sparse data: min(rows, cols) > %d (padded to 64) and so more than %d kept triples are not "
                         "supported" % (name, MAX_SPARSE_SIDE, MAX_SPARSE_SIDE))


def pinv(A, k=-1, eps=10 ** -8):                               # svd.py:27-45
    """Pseudo-inverse of the dense matrix A through SVD(A): V^T diag(1 / s_i for s_i > eps) U^T, float64."""
    if _is_sparse(A):
        raise TypeError("pinv: scipy.sparse data is not supported (dense data only)")
    svd_mdl = SVD(A, k=k)
    svd_mdl.factorize()
    s = svd_mdl.S.diagonal()
    inv = np.where(s > eps, 1.0 / np.where(s > eps, s, 1.0), 0.0)
    return np.dot(svd_mdl.V.T, inv[:, np.newaxis] * svd_mdl.U.T)


class SVD(object):
    """
    SVD(data, k=-1, rrank=0, crank=0)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> svd_mdl = SVD(data)
    >>> svd_mdl.factorize()
    """
    _EPS = 10 ** -8                                            # svd.py:74
    accept_sparse = False     # opt-in, per object: scipy.sparse data stays sparse on the device (module docstring)

    def __init__(self, data, k=-1, rrank=0, crank=0):          # svd.py:76-90
        self.data = data
        (self._rows, self._cols) = self.data.shape
        self._rrank = rrank if rrank > 0 else self._rows
        self._crank = crank if crank > 0 else self._cols
        self._k = k
        self._ctx = None
        self._on_device = None      # the (U, S, V) objects that the context's factors equal

    def _sparse_run(self):
        """`data` is a scipy.sparse matrix and this object takes it (accept_sparse set on the object itself)."""
        return bool(self.__dict__.get("accept_sparse", False)) and _is_sparse(self.data)

    def _check_supported(self):
        if _is_sparse(self.data) and not self._sparse_run():
            raise TypeError("SVD: scipy.sparse data is not supported (dense data only)")
        if self._sparse_run():
            check_sparse_limits("SVD", self._rows, self._cols, _dist.world().size)
        if _dist.world().size > 1:
            raise NotImplementedError("SVD: one rank only (a multi-rank world is not supported)")
        if min(self._rows, self._cols) > MAX_RANK:
            raise ValueError("SVD: min(rows, cols) > %d is not supported" % MAX_RANK)

    def _kept_triples(self):
        """svd.py:165,204: the reference's sparse branch keeps k triples for 0 < k < min(rows, cols) - 1; 0 = all."""
        short = min(self._rows, self._cols)
        return int(self._k) if 0 < self._k < short - 1 else 0

    def _context(self):
        if self._ctx is None:
            self._ctx = _lib.Context(_lib.ALGO_PCA, self._rows, self._cols, min(self._rows, self._cols),
                                     device=_dist.world().local_rank)
        return self._ctx

    def factorize(self):                                       # svd.py:110-244
        self._check_supported()
        sparse = self._sparse_run()
        arr = canonical_csr(self.data) if sparse else np.asarray(self.data[:, :])
        if arr.dtype == np.float64 and not self.__dict__.get("_warned_f64", False):
            self._warned_f64 = True
            warnings.warn("SVD: float64 data is rounded to float32 on the device (the Gram matrix of the rounded data is "
                          "formed in float64; DESIGN.md 3.14)", PrecisionWarning, stacklevel=2)
        ctx = self._context()
        if sparse:
            ctx.set_option("svd_num_triples", self._kept_triples())
            ctx.set_v_csr(arr.indptr.astype(np.int64), arr.indices.astype(np.int32), arr.data.astype(np.float32))
        else:
            ctx.set_v_dense(arr)
        rank = ctx.svd_decompose()
        U, S, V = ctx.svd_get(rank)
        self.U, self.S, self.V = U, np.diag(S), V
        self._on_device = (self.U, self.S, self.V)

    def frobenius_norm(self):                                  # svd.py:92-107
        """||data - U S V||_F of the data that factorize() saw."""
        self._check_supported()
        U, S, V = self.U, self.S, self.V                       # AttributeError before factorize(), as in the reference
        if self._ctx is None:
            raise AttributeError("SVD.frobenius_norm: factorize() has not run")
        ctx = self._context()
        cur = self._on_device
        if self._sparse_run():
            for name, have, want in zip("USV", (U, S, V), cur or (None, None, None)):
                if have is not want:
                    raise NotImplementedError("SVD.frobenius_norm on scipy.sparse data: %s was rebound; the error comes from the "
                                              "factors of the last factorize()" % name)
            return ctx.frobenius()
        if cur is None or U is not cur[0] or S is not cur[1] or V is not cur[2]:
            # the caller rebound a factor: the device takes W = U and H = S V of the arrays at hand
            k = ctx.k
            W = np.zeros((self._rows, k))
            H = np.zeros((k, self._cols))
            r = np.asarray(U).shape[1]
            if r > k:
                raise ValueError("SVD.frobenius_norm: U has more columns than min(rows, cols)")
            W[:, :r] = U
            H[:r] = np.dot(S, V)
            ctx.set_w(W)
            ctx.set_h(H)
            self._on_device = (U, S, V)
        return ctx.frobenius()
