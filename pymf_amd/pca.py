"""pymf_amd.PCA -- drop-in for pymf.PCA (reference pymf/pca.py) on MI355X.

W = the leading num_bases left singular vectors of the (centred) data, all of them when num_bases == 0 (pca.py:93-108);
H = W^T data (pca.py:90-91).  The decomposition is pymf_amd.SVD's: a float64 Gram matrix on the short side
of the float32 data, the float64 Jacobi solver, the projected side multiplied in float32.  `eigenvalues` holds the
SINGULAR values of the selected bases, as in the reference (pca.py:100,108).

The constructor centres as pca.py:73-82 does: `_data_orig`, `_meanv`, and `data = _data_orig - _meanv` in NumPy; the
centred array is what goes to the device.  init_w and init_h do nothing; factorize() always runs one iteration.

scipy.sparse data (opt-in: `mdl.accept_sparse = True`) with center_mean=False only: the centred data are dense (the reference
itself densifies there), so with center_mean=True factorize, update_w, update_h and frobenius_norm raise CentredSparseError: a
ValueError (center_mean=False is the value that works) that is also the TypeError such data raised before.  The switch is read
from the object, as SVD's.  The data
stay sparse on the device (pymf_amd.SVD's sparse path): only the leading num_bases triples are projected, W, H and
the error are float64 (H = W^T data over the stored entries, the error by the trace identity).  A W step that takes another
number of bases than the resident H has drops that H.  Limits there: min(rows, cols) <= 1024 after padding to 64.

Supported: dense data, resident, one rank, min(rows, cols) <= 2432, num_bases <= 2432; scipy.sparse data only as described
above.  Without that opt-in scipy.sparse data raises TypeError; streamed data (stream_rows) ValueError, a multi-rank world
NotImplementedError (on sparse data ValueError).
"""
import numpy as np

from . import _lib
from . import dist as _dist
from .nmf import NMF, _is_sparse
from .svd import MAX_RANK, canonical_csr, check_sparse_limits

__all__ = ["PCA", "CentredSparseError"]


class CentredSparseError(TypeError, ValueError):
    """PCA with center_mean=True on scipy.sparse data: the data are not taken as they are (TypeError, as without the flag), and
    center_mean=False is the argument value under which they are (ValueError)."""


class _WideFactors(object):
    """The context's W and H are max(min(rows, cols), num_bases) bases wide (the decomposition may find any rank up to the
    short side); the class's W has as many columns as it has: zero padded on the way in, cut on the way out."""

    def __init__(self, ctx):
        self._c = ctx
        self.cols = 0                                          # columns of the W that the device holds

    def __getattr__(self, name):
        return getattr(self._c, name)

    def _padded(self, A, axis):
        A = np.asarray(A)
        if A.shape[axis] > self._c.k:
            raise ValueError("PCA: a factor with %d bases does not fit the context's %d" % (A.shape[axis], self._c.k))
        shape = (A.shape[0], self._c.k) if axis == 1 else (self._c.k, A.shape[1])
        P = np.zeros(shape, dtype=A.dtype if A.dtype in (np.float32, np.float64) else np.float64)
        P[:A.shape[0], :A.shape[1]] = A
        return P

    def set_w(self, W):
        self._c.set_w(self._padded(W, 1))
        self.cols = np.asarray(W).shape[1]

    def set_h(self, H):
        self._c.set_h(self._padded(H, 0))

    def get_w_into(self, out):
        return False

    def get_h_into(self, out):
        return False


class PCA(NMF):
    """
    PCA(data, num_bases=0, center_mean=True)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> pca_mdl = PCA(data, num_bases=2)
    >>> pca_mdl.factorize()

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5], [1.2]])
    >>> pca_mdl = PCA(data, num_bases=2)
    >>> pca_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> pca_mdl.factorize(compute_w=False)
    """
    _SHIPPED = True
    _ALGO = _lib.ALGO_PCA
    accept_sparse = False     # opt-in, per object: scipy.sparse data stays sparse on the device (center_mean=False only; module docstring)
    _NITER = 1                                                 # pca.py:133
    _SKIP_MISSING_FACTORS = True                               # update_w needs neither factor, update_h no H (both are written whole)

    def __init__(self, data, num_bases=0, center_mean=True):
        NMF.__init__(self, data, num_bases=num_bases)
        self._center_mean = center_mean                        # pca.py:73-82
        if self._center_mean and not _is_sparse(data):
            self._data_orig = data
            self._meanv = self._data_orig[:, :].mean(axis=1).reshape(data.shape[0], -1)
            self.data = self._data_orig - self._meanv
        else:
            self.data = data

    def _check_supported(self):
        name = type(self).__name__
        if _is_sparse(self.data):
            if not self._sparse_run():
                raise TypeError("%s: scipy.sparse data is not supported (dense data only)" % name)
            if self._center_mean:
                raise CentredSparseError("%s on scipy.sparse data: the centred data are dense; pass center_mean=False" % name)
            check_sparse_limits(name, self._data_dimension, self._num_samples, self._world().size)
        if self.stream_rows or self._stream_rows():
            raise ValueError("%s: streamed data (stream_rows) is not supported: the Gram matrix needs the data resident" % name)
        if self._world().size > 1:
            raise NotImplementedError("%s: one rank only (a multi-rank world is not supported)" % name)
        if min(self._data_dimension, self._num_samples) > MAX_RANK or self._num_bases > MAX_RANK:
            raise ValueError("%s: min(rows, cols) and num_bases beyond %d are not supported" % (name, MAX_RANK))

    def _sparse_run(self):
        """`data` is a scipy.sparse matrix and this object takes it (accept_sparse; PCA itself, not its subclasses)."""
        return bool(self.__dict__.get("accept_sparse", False)) and type(self)._ALGO == _lib.ALGO_PCA and _is_sparse(self.data)

    def _upload_sparse(self, ctx):
        self._check_supported()
        csr = canonical_csr(self.data)
        self._warn_if_float64(csr.data)
        ctx.set_v_csr(csr.indptr.astype(np.int64), csr.indices.astype(np.int32), csr.data.astype(np.float32))

    def _context(self):
        if self._ctx is None:
            k = max(min(self._data_dimension, self._num_samples), self._num_bases, 1)
            ctx = _dist.make_context(self._ALGO, self._data_dimension, self._num_samples, k)
            ctx.set_option("pca_num_bases", max(0, self._num_bases))
            ctx.set_option("svd_num_triples", min(max(0, self._num_bases), 1024))   # (what a decomposition of sparse data keeps)
            self._ctx = _WideFactors(ctx)
        return self._ctx

    def _took_w(self, ctx):
        """Behind a W step on the device: how many bases it took, and their singular values (pca.py:100-108)."""
        rank = ctx.svd_rank()
        ctx.cols = min(self._num_bases, rank) if self._num_bases > 0 else rank
        self.eigenvalues = ctx.svd_get(rank, want="S")[1][:ctx.cols]

    def _download(self, ctx, name, cur):
        if name == "H":                                        # pca.py:91 binds a new array
            return ctx.get_h64()[:ctx.cols].copy()
        return ctx.svd_get(ctx.svd_rank(), want="U")[0][:, :ctx.cols].copy()   # pca.py:107: columns of U, float64

    def _pull(self, ctx, moved):                               # (there may be no host array yet: init_w / init_h do nothing)
        for name in moved:
            self._host_stale.discard(name)
            self._host_is_current(name, self._download(ctx, name, None))

    # ---- the reference's hooks ------------------------------------------------------------------------------------
    def init_h(self):                                          # pca.py:84-85
        pass

    def init_w(self):                                          # pca.py:87-88
        pass

    def update_w(self):                                        # pca.py:93-108
        self._check_supported()
        ctx = self._sync_to_device()
        ctx.update_w()
        self._took_w(ctx)
        self._pull(ctx, ("W",))

    def update_h(self):                                        # pca.py:90-91
        self._check_supported()
        if not self._has("W"):
            raise AttributeError("'%s' object has no attribute 'W'" % type(self).__name__)
        ctx = self._sync_to_device()
        ctx.update_h()
        self._pull(ctx, ("H",))

    def frobenius_norm(self):
        self._check_supported()
        if self._sparse_run():                                 # (NMF's returns the reference's -123456 sentinel on sparse data)
            if not (self._has('H') and self._has('W')):
                return -123456
            return self._sync_to_device().frobenius()
        return NMF.frobenius_norm(self)

    def factorize(self, show_progress=False, compute_w=True, compute_h=True, compute_err=True, niter=1):
        """Factorize s.t. WH = data; always one iteration (pca.py:110-135)."""
        self._check_supported()
        NMF.factorize(self, niter=1, show_progress=show_progress, compute_w=compute_w, compute_h=compute_h,
                      compute_err=compute_err)

    def _after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call=None):
        if compute_w and result[1] > 0:
            self._took_w(ctx)
        NMF._after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call)
