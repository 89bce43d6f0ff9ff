"""pymf_amd.GREEDY -- drop-in for pymf.GREEDY (reference pymf/greedy.py, Civril and Magdon-Ismail) on MI355X, dense data.

Deterministic column selection: W is num_bases columns of the data, chosen one after the other so that they best reproduce
the leading singular subspace B = (U S)[:, :num_bases] of the data; H = pinv(W) data.  The reference normalises and deflates
the whole matrix in every round (greedy.py:122-158).  Here the data are read only: with Q an orthonormal
basis of the columns chosen so far and B' = (I - Q Q^T) B, the reference's score of column v_j is
|B'^T v_j|^2 / (|v_j|^2 - |Q^T v_j|^2).  For rows <= cols a round is one pass over the float32 data on the fp32 MFMA with the
argmax in its epilogue and one small float64 step, all rounds enqueued back to back; for rows > cols the whole loop runs in
Gram space on the float64 cols x cols Gram matrix.  B comes from the eigenpairs of the float64 Gram matrix on the short side,
as SVD's does; the `k` argument is ignored for dense data, as in the reference (svd.py).  `select` lists the chosen columns in
selection order (Python ints), W holds bit-exact copies of them in a new array of the data's dtype, H is float64.

When num_bases exceeds the numerical rank of the data, the reference goes on selecting on rounding noise (it normalises
residual columns of size 1e-16).  Here a column whose residual norm^2 is <= 0 or <= 512 unit roundoffs of its norm^2
(float32 roundoffs for rows <= cols, float64 ones in Gram space) scores 0; once every column does, the lowest index not yet
chosen is taken.  The selections made while the residuals are above that level are the reference's, the later ones are valid
column indices but need not be.

factorize() has the reference's loop (nmf.py:182-202): both updates are deterministic, so with niter >= 3 and compute_err
the convergence test stops it at i = 2 and ferr keeps two entries.  init_w and init_h are NMF's, so NumPy's global stream
is consumed as in the reference.

Supported: dense data, resident, one rank, num_bases <= 64, min(rows, cols) <= 2432.  scipy.sparse data raises TypeError,
streamed data (stream_rows) ValueError, a multi-rank world NotImplementedError, more bases or a longer short side ValueError.

scipy.sparse data (opt-in: `mdl.accept_sparse = True`, the switch NMF, CUR and SVD have; GREEDY only -- GREEDYCUR keeps
refusing).  The matrix is converted once to canonical CSR (tocsr(), duplicates summed, indices sorted, float32 values, stored
zeros kept) and stays sparse on the device through all rounds: the score above is evaluated on stored entries
(k_greedy_csr_pass), W is scattered from them, H = pinv(W) data and the error are formed in float64 without a
dense image.  factorize(), update_w(), update_h() and frobenius_norm() give what the dense run on toarray() gives: `select`,
bit-exact columns in a dense W of the data's dtype, a dense float64 H, ferr filled (compute_err=True works; NMF's -123456
sentinel is not used here).  Limits on top of the above: min(rows, cols), padded to 64, at most 1024 (ValueError).
Deliberate deviations from the reference's sparse branch (greedy.py:115-141): it subtracts a rank-one matrix from the data in
every round, so its matrix is dense after the first selection -- here the data are never written; W and H come back dense;
and the `k` argument stays ignored: all eigenpairs of the short side come from the Jacobi solver, where the reference asks
ARPACK for k = num_bases triples -- the leading num_bases columns of B are the same.  ferr is the float64 identity
||data||^2 - 2 <W^T data, H> + <W^T W, H H^T>, clamped at 0.
"""
import numpy as np

from . import _lib
from .nmf import NMF, _is_sparse
from .svd import MAX_SPARSE_SIDE, canonical_csr

__all__ = ["GREEDY"]

MAX_BASES = 64        # PMF_GREEDY_MAX_BASES (pmf_greedy.h)
MAX_SHORT_SIDE = 2432 # PMF_SVD_MAX_RANK (pmf_svd.h)


class GREEDY(NMF):
    """
    GREEDY(data, k=-1, num_bases=4)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> greedy_mdl = GREEDY(data, num_bases=2)
    >>> greedy_mdl.factorize()

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5, 1.3], [1.2, 0.3]])
    >>> greedy_mdl = GREEDY(data, num_bases=2)
    >>> greedy_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> greedy_mdl.factorize(compute_w=False)
    """
    _SHIPPED = True
    _ALGO = _lib.ALGO_GREEDY
    _SKIP_MISSING_FACTORS = True                               # update_w needs neither factor, update_h no H (both are written whole)
    accept_sparse = False     # opt-in, per object: scipy.sparse data stays sparse on the device (module docstring)
    _TAKES_SPARSE = True      # GREEDY itself; a class without the sparse device path says False

    def __init__(self, data, k=-1, num_bases=4):               # greedy.py:75-80
        NMF.__init__(self, data, num_bases=num_bases)
        self._k = k
        if self._k == -1:
            self._k = num_bases

    def _sparse_run(self):
        """`data` is a scipy.sparse matrix and this object takes it (accept_sparse)."""
        return bool(self.accept_sparse) and self._TAKES_SPARSE and _is_sparse(self.data)

    def _upload_sparse(self, ctx):
        self._check_supported()
        csr = canonical_csr(self.data)
        self._warn_if_float64(csr.data)
        ctx.set_v_csr(csr.indptr.astype(np.int64), csr.indices.astype(np.int32), csr.data.astype(np.float32))

    def _check_supported(self):
        name = type(self).__name__
        if _is_sparse(self.data):
            if not self._sparse_run():
                raise TypeError("%s: scipy.sparse data is not supported (dense data only)" % name)
            if -(-min(self._data_dimension, self._num_samples) // 64) * 64 > MAX_SPARSE_SIDE:
                raise ValueError("%s on scipy.sparse data: min(rows, cols) > %d (padded to 64) is not supported" % (name, MAX_SPARSE_SIDE))
        if self.stream_rows or self._stream_rows():
            raise ValueError("%s: streamed data (stream_rows) is not supported: the selection needs the data resident" % name)
        if self._world().size > 1:
            raise NotImplementedError("%s: one rank only (a multi-rank world is not supported)" % name)
        if self._num_bases > MAX_BASES:
            raise ValueError("%s: num_bases > %d is not supported" % (name, MAX_BASES))
        if min(self._data_dimension, self._num_samples) > MAX_SHORT_SIDE:
            raise ValueError("%s: min(rows, cols) > %d is not supported" % (name, MAX_SHORT_SIDE))

    def _download(self, ctx, name, cur):
        if name == "H":                                        # greedy.py:86: the float64 product
            return ctx.get_h64()
        # greedy.py:167-170 rebinds W to columns of the data: a new array of the data's dtype
        dt = self.data.dtype if np.issubdtype(getattr(self.data, "dtype", np.float64), np.floating) else np.float64
        if dt == np.float32:
            return ctx.get_w().astype(dt, copy=False)
        if self._sparse_run():                                 # (the caller's values, not their float32 rounding, as on dense data)
            return np.ascontiguousarray(self.data.tocsc()[:, self.select].toarray()).astype(dt, copy=False)
        return np.ascontiguousarray(np.asarray(self.data[:, :])[:, self.select]).astype(dt, copy=False)

    def _take_select(self, ctx):
        self.select = [int(s) for s in ctx.get_select()]

    # ---- the reference's hooks ------------------------------------------------------------------------------------
    def update_w(self):                                        # greedy.py:88-170
        self._check_supported()
        t0 = _now()
        ctx = self._sync_to_device()
        ctx.update_w()
        self._take_select(ctx)
        self._t = np.full(self._num_bases, _now() - t0)        # (the rounds run back to back on the device: one time for all)
        if not self._has("W"):
            self.__dict__["_W"] = np.zeros((self._data_dimension, self._num_bases), dtype=np.float32)   # (the host array that the new W replaces)
        self._pull(ctx, ("W",))

    def update_h(self):                                        # greedy.py:82-86
        self._check_supported()
        if not self._has("W"):
            raise AttributeError("'%s' object has no attribute 'W'" % type(self).__name__)
        ctx = self._sync_to_device()
        ctx.update_h()
        if not self._has("H"):
            self.__dict__["_H"] = np.zeros((self._num_bases, self._num_samples))   # (the host array that the new H replaces)
        self._pull(ctx, ("H",))

    def frobenius_norm(self):
        self._check_supported()
        if self._sparse_run():                                 # (NMF's returns the reference's -123456 sentinel on sparse data)
            if not (self._has('H') and self._has('W')):
                return -123456
            return self._sync_to_device().frobenius()
        return NMF.frobenius_norm(self)

    def factorize(self, niter=1, show_progress=False, compute_w=True, compute_h=True, compute_err=True):
        """Factorize s.t. WH = data (nmf.py:141-202)."""
        self._check_supported()
        self._t0 = _now()
        NMF.factorize(self, niter=niter, show_progress=show_progress, compute_w=compute_w, compute_h=compute_h,
                      compute_err=compute_err)

    def _after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call=None):
        if compute_w and result[1] > 0:
            self._take_select(ctx)
            self._t = np.full(self._num_bases, _now() - self._t0)
        NMF._after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call)


def _now():
    import time
    return time.time()
