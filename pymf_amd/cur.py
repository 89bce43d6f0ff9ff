"""pymf_amd.CUR -- drop-in for pymf.CUR (reference pymf/cur.py) on MI355X, dense data.

CUR samples rows and columns of the data with probabilities proportional to their squared norms and factorises
data ~ C U R with C = data[:, cid] diag(sqrt(ccnt)), R = diag(sqrt(rcnt)) data[rid, :] and U = pinv(C) data pinv(R)
(cur.py:84-138).  On the device the squared norms come from one read of the float32 data in float64 (k_cur_sqnorms), and
U is computed as (C^T C)^+ (C^T data R^T) (R R^T)^+: the two small Gram matrices and the middle product, the one pass over
the data, run in float64 on the float64 MFMA (one kernel, k_prod_f64, with two tile maps), the pseudo-inverses come from the float64 Jacobi
solver with svd.py's 1e-8 cut on the eigenvalues.  U (= C), S (= the middle factor) and V (= R) come back as
float64 arrays, as the reference returns them.

The draws stay on the host and use NumPy's global stream exactly as the reference does (rows first, then columns, one
`np.random.rand()` per draw), so a caller who seeds `np.random` gets the reference's indices.

As in the reference, `CUR.__init__` hands `crank=rrank` to `SVD.__init__` (cur.py:60): the `crank` argument is ignored and
`_crank` follows `rrank`; `rrank = 0` means all rows and all columns.

`computeUCR()` works from whatever `_rid`, `_cid`, `_rcnt` and `_ccnt` hold (unsorted, repeated and negative indices
included): set them by hand, or let a subclass such as CMD set them.

Supported: dense data, one rank, at most 128 sampled rows and 128 sampled columns.  scipy.sparse data raises TypeError, a
multi-rank world NotImplementedError, more rows or columns ValueError.

scipy.sparse data (opt-in: `mdl.accept_sparse = True`, the switch NMF has; CUR and CMD only).  The matrix is converted once
to canonical CSR (tocsr(), duplicates summed, indices sorted, float32 values) and stays sparse on the device: the norms, the
gathers and the middle product read stored entries only (k_cur_csr_sqnorms, k_cur_csr_gather, k_cur_csr_mid),
the rest is the dense path.  factorize(), sample_probability() and computeUCR() give what the dense run on toarray() gives,
with the same draws.  Deliberate deviations from the reference's sparse branch: U, S, V come back as dense float64 arrays (the
reference returns sparse C and R), and pinv is not routed through ARPACK with k = min(dim) - 1, which silently drops the
smallest singular pair -- the yardstick is the dense path.  frobenius_norm() is evaluated in float64 without a dense image,
ferr^2 = ||data||^2 - 2 <U, C^T data R^T> + <(C^T C) U, U (R R^T)> (clamped at 0), from what computeUCR() formed; it needs
the factors of that call: a rebound U, S or V raises NotImplementedError.
"""
import warnings

import numpy as np

from . import _lib
from . import dist as _dist
from .nmf import PrecisionWarning, _is_sparse
from .svd import SVD

__all__ = ["CUR"]

MAX_RANK = 128    # PMF_CUR_MAX_RANK (pmf_cur.h)


class CUR(SVD):
    """
    CUR(data, k=-1, rrank=0, crank=0)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> cur_mdl = CUR(data, rrank=1, crank=2)
    >>> cur_mdl.factorize()
    """

    accept_sparse = False     # opt-in: scipy.sparse data stays sparse on the device (CUR and CMD)
    _TAKES_SPARSE = True      # the subclasses without a sparse device path switch it off

    def __init__(self, data, k=-1, rrank=0, crank=0):          # cur.py:59-66
        SVD.__init__(self, data, k=k, rrank=rrank, crank=rrank)
        self._rset = range(self._rows)
        self._cset = range(self._cols)
        self._fresh = False         # the context holds the data of this factorize() call

    def _sparse_run(self):
        """`data` is a scipy.sparse matrix and this object takes it (accept_sparse; CUR and CMD)."""
        return bool(self.accept_sparse) and self._TAKES_SPARSE and _is_sparse(self.data)

    def _check_supported(self):
        if _is_sparse(self.data) and not self._sparse_run():
            raise TypeError("CUR: scipy.sparse data is not supported (dense data only; CUR and CMD take it with accept_sparse = True)")
        if _dist.world().size > 1:
            raise NotImplementedError("CUR: one rank only (a multi-rank world is not supported)")

    def _context(self, k=None):
        if self._ctx is not None and k is not None and k > self._ctx.k:
            self._ctx.close()
            self._ctx = None
        if self._ctx is None:
            k = max(k or 1, min(max(self._rrank, self._crank), MAX_RANK))
            self._ctx = _lib.Context(_lib.ALGO_CUR, self._rows, self._cols, k, device=_dist.world().local_rank)
            self._on_device = None
        return self._ctx

    def _upload(self):
        self._check_supported()
        sparse = self._sparse_run()
        if sparse:
            arr = self.data.tocsr()
            if not arr.has_canonical_format:
                if arr is self.data:
                    arr = arr.copy()                           # (the caller's matrix keeps its entries as they are)
                arr.sum_duplicates()
        else:
            arr = np.asarray(self.data[:, :])
        if arr.dtype == np.float64 and not self.__dict__.get("_warned_f64", False):
            self._warned_f64 = True
            warnings.warn("CUR: float64 data is rounded to float32 on the device (norms, Gram matrices and the middle "
                          "product of the rounded data are formed in float64; DESIGN.md 3.15)", PrecisionWarning, stacklevel=3)
        ctx = self._context()
        if sparse:
            ctx.set_v_csr(arr.indptr.astype(np.int64), arr.indices.astype(np.int32), arr.data.astype(np.float32))
        else:
            ctx.set_v_dense(arr)
        return ctx

    def sample(self, s, probs):                                # cur.py:69-82
        prob_rows = np.cumsum(probs.flatten())
        temp_ind = np.zeros(s, np.int32)
        for i in range(s):
            v = np.random.rand()
            hit = np.where(prob_rows >= v)[0]
            if hit.shape[0] == 0:
                # (the reference stores len(prob_rows) here and fails with IndexError when it indexes the data)
                raise IndexError("CUR.sample: a draw exceeds the last cumulative probability")
            temp_ind[i] = hit[0]
        return np.sort(temp_ind)

    def sample_probability(self):                              # cur.py:84-97
        ctx = self._upload()
        self._fresh = True
        prow, pcol = ctx.cur_sqnorms()
        prow /= prow.sum()
        pcol /= pcol.sum()
        return (prow.reshape(-1, 1), pcol.reshape(-1, 1))

    @staticmethod
    def _index_list(idx, cnt, extent, what):
        idx = np.asarray(idx).ravel()
        cnt = np.asarray(cnt, dtype=np.float64).ravel()
        if idx.shape != cnt.shape or idx.shape[0] < 1:
            raise ValueError("CUR.computeUCR: %s indices and counts must be non-empty and of equal length" % what)
        if idx.shape[0] > MAX_RANK:
            raise ValueError("CUR: more than %d sampled %s are not supported" % (MAX_RANK, what))
        idx = idx.astype(np.int64)
        if np.any(idx < -extent) or np.any(idx >= extent):
            raise IndexError("CUR.computeUCR: %s index out of range" % what)
        icnt = np.rint(cnt).astype(np.int32)
        if np.any(icnt < 1) or not np.array_equal(icnt.astype(np.float64), cnt):
            raise ValueError("CUR.computeUCR: %s counts must be positive integers" % what)
        return idx.astype(np.int32), icnt

    def computeUCR(self):                                      # cur.py:99-120
        self._check_supported()
        rid, rcnt = self._index_list(self._rid, self._rcnt, self._rows, "rows")
        cid, ccnt = self._index_list(self._cid, self._ccnt, self._cols, "columns")
        need = max(rid.shape[0], cid.shape[0])
        if self._ctx is None or need > self._ctx.k:
            self._fresh = False
            self._context(need)
        if not self._fresh:
            self._upload()
        self._fresh = False
        ctx = self._context()
        ctx.cur_compute(rid, rcnt, cid, ccnt)
        self._C, self._U, self._R = ctx.cur_get()
        # set some standard (with respect to SVD) variable names
        self.U = self._C
        self.S = self._U
        self.V = self._R
        self._on_device = (self.U, self.S, self.V)

    def frobenius_norm(self):                                  # svd.py:92-107
        """||data - U S V||_F of the data that computeUCR() saw; on sparse data from the trace identity (module docstring)."""
        if not self._sparse_run():
            return SVD.frobenius_norm(self)
        self._check_supported()
        U, S, V = self.U, self.S, self.V                       # AttributeError before factorize(), as in the reference
        cur = self._on_device
        if self._ctx is None or cur is None:
            raise AttributeError("CUR.frobenius_norm: computeUCR() has not run")
        for name, have, want in zip("USV", (U, S, V), cur):
            if have is not want:
                raise NotImplementedError("CUR.frobenius_norm on scipy.sparse data: %s was rebound; the error comes from the "
                                          "factors of the last computeUCR()" % name)
        return self._ctx.cur_ferr()

    def _check_ranks(self):
        if self._rrank > MAX_RANK or self._crank > MAX_RANK:
            raise ValueError("CUR: rrank > %d is not supported (rrank = 0 samples as many rows and columns as the data have)" % MAX_RANK)

    def factorize(self):                                       # cur.py:122-138
        self._check_supported()
        self._check_ranks()
        [prow, pcol] = self.sample_probability()
        self._rid = self.sample(self._rrank, prow)
        self._cid = self.sample(self._crank, pcol)

        self._rcnt = np.ones(len(self._rid))
        self._ccnt = np.ones(len(self._cid))

        self.computeUCR()
