"""pymf_amd.AA -- drop-in for pymf.AA (reference pymf/aa.py) on MI355X.

Archetypal analysis: W = data beta^T with beta >= 0 and rows summing to 1, H >= 0 with columns summing to 1, by alternating
least squares.  update_w projects every column of W_hat = data pinv(H) onto the convex hull of the data columns
(aa.py:113-134); on the device that is column generation in data space -- rounds of one pricing pass over the resident data
and one small float64 solve per base, the n x n Hessian of the reference's QPs is never formed.  update_h
is the simplex-constrained step that SIVM inherits (aa.py:93-111).  `beta` (num_bases x num_samples,
float64) holds the weights of the last W step; where num_samples > data_dimension they are not unique, W is.

Supported: dense data, resident, one rank, num_bases <= 64, min(data_dimension + 1, num_samples) <= 128 (a base's corral of
data columns).  scipy.sparse data raises TypeError, streamed data (stream_rows) ValueError, a multi-rank world
NotImplementedError, more than 64 bases ValueError, a shape beyond the corral bound ValueError.  An H without full row rank
makes update_w raise (W_hat is formed through inv(H H^T), which equals the reference's pinv only then); a W whose Gram
matrix is not positive definite makes update_h raise.
"""
import numpy as np

from . import _lib
from .nmf import NMF, _is_sparse

__all__ = ["AA"]


class AA(NMF):
    """
    AA(data, num_bases=4)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> aa_mdl = AA(data, num_bases=2)
    >>> aa_mdl.factorize(niter=5)

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5], [1.2]])
    >>> aa_mdl = AA(data, num_bases=2)
    >>> aa_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> aa_mdl.factorize(niter=5, compute_w=False)
    """
    _SHIPPED = True
    _ALGO = _lib.ALGO_AA
    _MAX_BASES = 64
    _MAX_CORRAL = 128

    def _check_supported(self):
        name = type(self).__name__
        if _is_sparse(self.data):
            raise TypeError("%s: scipy.sparse data is not supported (dense data only)" % name)
        if self.stream_rows or self._stream_rows():
            raise ValueError("%s: streamed data (stream_rows) is not supported: the pricing passes need the data resident" % name)
        if self._world().size > 1:
            raise NotImplementedError("%s: one rank only (a multi-rank world is not supported)" % name)
        if self._num_bases > self._MAX_BASES:
            raise ValueError("%s: num_bases > %d is not supported" % (name, self._MAX_BASES))
        if min(self._data_dimension + 1, self._num_samples) > self._MAX_CORRAL:
            raise ValueError("%s: min(data_dimension + 1, num_samples) > %d (the corral bound) is not supported"
                             % (name, self._MAX_CORRAL))

    def _download(self, ctx, name, cur):
        if name == "H":                                        # aa.py:101 fills the float64 H of init_h
            return ctx.get_h64()
        # aa.py:134 rebinds W to data beta^T: a new array of the data's dtype
        dt = self.data.dtype if np.issubdtype(getattr(self.data, "dtype", np.float64), np.floating) else np.float64
        return ctx.get_w().astype(dt, copy=False)

    def _take_beta(self, ctx):
        self.beta = ctx.get_beta()

    # ---- the reference's hooks ------------------------------------------------------------------------------------
    def init_h(self):                                          # aa.py:83-85
        self.H = np.random.random((self._num_bases, self._num_samples))
        self.H /= self.H.sum(axis=0)

    def init_w(self):                                          # aa.py:87-91: both draws, in this order; the second W stays
        self.beta = np.random.random((self._num_bases, self._num_samples))
        self.beta /= self.beta.sum(axis=0)
        self.W = np.random.random((self._data_dimension, self._num_bases))

    def update_w(self):                                        # aa.py:113-134
        self._check_supported()
        ctx = self._sync_to_device()
        ctx.update_w()
        self._take_beta(ctx)
        self._pull(ctx, ("W",))

    def update_h(self):                                        # aa.py:93-111
        self._check_supported()
        ctx = self._sync_to_device()
        ctx.update_h()
        self._pull(ctx, ("H",))

    def frobenius_norm(self):
        self._check_supported()
        return NMF.frobenius_norm(self)

    def factorize(self, niter=1, show_progress=False, compute_w=True, compute_h=True, compute_err=True):
        """Factorize s.t. WH = data (nmf.py:141-202)."""
        self._check_supported()
        NMF.factorize(self, niter=niter, show_progress=show_progress, compute_w=compute_w, compute_h=compute_h,
                      compute_err=compute_err)

    def _after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call=None):
        NMF._after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call)
        if compute_w and result[1] > 0:
            self._take_beta(ctx)
