"""pymf_amd.SIVM -- drop-in for pymf.SIVM (reference pymf/sivm.py) on MI355X.

Simplex volume maximisation: W is a selection of num_bases columns of the data, chosen one after the other so that the
volume of the simplex they span grows fastest (sivm.py:145-201); every column of H then solves
min ||data[:, c] - W h||, h >= 0, sum(h) = 1 (AA.update_h, aa.py:93-111).  On the device update_w is num_bases + 2
('fastmap') or num_bases ('origin') passes over the resident data enqueued back to back, update_h a bracketing secant on the
multiplier of the sum constraint over rounds of non-negative QPs.  `select` lists the chosen columns in
selection order; under init='origin' its first entry is -1, which the reference uses as a Python index: that column of W
is the LAST data column.

factorize() always runs one iteration (sivm.py:203-228).  init_w and init_h give zeros, as in the reference.

Supported: dense or scipy.sparse data, resident, one rank, num_bases <= 64, data_dimension <= 16384, dist_measure 'l2', 'l1'
or 'cosine'.  Streamed data (stream_rows) raises ValueError, a multi-rank world NotImplementedError, more than 64 bases
ValueError, the measures 'kl', 'abs_cosine' and 'weighted_abs_cosine' NotImplementedError.  A W whose Gram matrix is not
positive definite (duplicate columns, or num_bases > data_dimension) makes update_h raise: H is not unique.

scipy.sparse data (any format; the reference takes it under 'l2', sivm.py:110-120) is converted once to CSC with sorted
indices, summed duplicates and float32 values and stays sparse on the device: the passes read stored entries only (DESIGN.md
3.23).  Semantics are those of the dense run on data.toarray(), for all three measures and both inits; `select` and the float64
H are as on dense data.  Deviations from the reference: W is a dense ndarray of the data's float dtype (the reference binds a
sparse slice that its own update_h cannot use); a column measured against itself has distance exactly 0, so it is never picked
a second time (the reference's expansion form can leave sqrt(<0) = NaN there, which np.argmax then picks).  There is no error
norm: factorize(compute_err=True) -- the default -- raises TypeError on sparse data and frobenius_norm() returns the
reference's -123456 (nmf.py:109-112); pass compute_err=False.  The subclasses (LAESA, GMAP, SIVM_SGREEDY, SIVM_GSAT) keep raising
TypeError on sparse data.
"""
import numpy as np

from . import _lib
from .nmf import NMF, _fingerprint, _is_sparse

__all__ = ["SIVM"]

_METRICS = {"l2": 0, "l1": 1, "cosine": 2}
_UNSUPPORTED_METRICS = ("kl", "abs_cosine", "weighted_abs_cosine")
_INITS = {"fastmap": 0, "origin": 1}


class SIVM(NMF):
    """
    SIVM(data, num_bases=4, dist_measure='l2', init='fastmap')

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> sivm_mdl = SIVM(data, num_bases=2)
    >>> sivm_mdl.factorize()

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5, 1.3], [1.2, 0.3]])
    >>> sivm_mdl = SIVM(data, num_bases=2)
    >>> sivm_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> sivm_mdl.factorize(compute_w=False)
    """
    _SHIPPED = True
    _ALGO = _lib.ALGO_SIVM
    _NITER = 1                                                 # sivm.py:76-78
    _MAX_BASES = 64
    _SKIP_MISSING_FACTORS = True                               # update_w needs neither factor, update_h no H (both are written whole)
    _TAKES_SPARSE = True                                       # SIVM itself takes scipy.sparse data; its subclasses say False

    def __init__(self, data, num_bases=4, dist_measure='l2', init='fastmap'):
        NMF.__init__(self, data, num_bases=num_bases)
        self._dist_measure = dist_measure
        self._init = init

    def _check_supported(self):
        name = type(self).__name__
        if _is_sparse(self.data) and not self._TAKES_SPARSE:
            raise TypeError("%s: scipy.sparse data is not supported (dense data only)" % name)
        if self.stream_rows or self._stream_rows():
            raise ValueError("%s: streamed data (stream_rows) is not supported: the selection passes need the data resident" % name)
        if self._world().size > 1:
            raise NotImplementedError("%s: one rank only (a multi-rank world is not supported)" % name)
        if self._num_bases > self._MAX_BASES:
            raise ValueError("%s: num_bases > %d is not supported" % (name, self._MAX_BASES))
        if self._dist_measure in _UNSUPPORTED_METRICS:
            raise NotImplementedError("%s: dist_measure '%s' is not supported ('l2', 'l1' and 'cosine' are)" % (name, self._dist_measure))
        if self._dist_measure not in _METRICS:
            raise ValueError("%s: unknown dist_measure %r" % (name, self._dist_measure))
        if self._init not in _INITS:
            raise ValueError("%s: init must be 'fastmap' or 'origin', not %r" % (name, self._init))

    def _context(self):
        fresh = self._ctx is None
        ctx = NMF._context(self)
        if fresh:
            ctx.set_option("sivm_metric", _METRICS[self._dist_measure])
            ctx.set_option("sivm_init", _INITS[self._init])
        return ctx

    def _csc(self):
        """`data` as the CSC matrix that goes to the device: sorted indices, duplicates summed, float32 values; explicit zeros
        stay stored.  The caller's matrix keeps its entries as they are."""
        csc = self.data.tocsc()
        if not csc.has_canonical_format:
            if csc is self.data:
                csc = csc.copy()
            csc.sum_duplicates()                               # (sorts the indices as well)
        return csc

    def _upload_data(self, ctx):
        if not _is_sparse(self.data):
            return NMF._upload_data(self, ctx)
        same_obj = self._v_src is self.data
        if same_obj and not self.check_data:
            return
        # the digest is taken of the caller's own arrays (whatever the format): an unchanged matrix costs no conversion
        own = [getattr(self.data, a) for a in ("indptr", "indices", "row", "col", "offsets", "data") if isinstance(getattr(self.data, a, None), np.ndarray)]
        if self.check_data and len(own) < 2:                   # (a format without plain arrays, LIL or DOK: digest the converted ones)
            own = None
        csc = self._csc() if own is None or not self.check_data else None
        if csc is not None and own is None and self.check_data:
            own = [csc.indptr, csc.indices, csc.data]
        fp = (self.data.shape, getattr(self.data, "format", None)) + tuple(_fingerprint(x) for x in own) if self.check_data else None
        if same_obj and fp == self._v_fp:
            return
        if csc is None:
            csc = self._csc()
        self._uploaded = True
        self._warn_if_float64(csc.data)
        ctx.set_v_csc(csc.indptr, csc.indices, csc.data)
        self._v_src = self.data
        self._v_fp = fp

    def _download(self, ctx, name, cur):
        if name == "H":                                        # aa.py:101 fills the float64 H of init_h
            return ctx.get_h64()
        # sivm.py:198-201 rebinds W to columns of the data: a new array of the data's dtype
        dt = self.data.dtype if np.issubdtype(getattr(self.data, "dtype", np.float64), np.floating) else np.float64
        return ctx.get_w().astype(dt, copy=False)

    def _take_select(self, ctx):
        self.select = [int(s) for s in ctx.get_select()]

    # ---- the reference's hooks ------------------------------------------------------------------------------------
    def init_h(self):                                          # sivm.py:139-140
        self.H = np.zeros((self._num_bases, self._num_samples))

    def init_w(self):                                          # sivm.py:142-143
        self.W = np.zeros((self._data_dimension, self._num_bases))

    def update_w(self):                                        # sivm.py:168-201
        self._check_supported()
        if not self._has("W"):
            self.init_w()                                      # (the host array that the new W replaces)
        ctx = self._sync_to_device()
        ctx.update_w()
        self._take_select(ctx)
        self._pull(ctx, ("W",))

    def update_h(self):                                        # aa.py:93-111
        self._check_supported()
        if not self._has("W"):
            raise AttributeError("'%s' object has no attribute 'W'" % type(self).__name__)
        if not self._has("H"):
            self.init_h()
        ctx = self._sync_to_device()
        ctx.update_h()
        self._pull(ctx, ("H",))

    def frobenius_norm(self):
        self._check_supported()
        return NMF.frobenius_norm(self)                        # (sparse data: the reference's -123456, nmf.py:109-112)

    def factorize(self, show_progress=False, compute_w=True, compute_h=True, compute_err=True, niter=1):
        """Factorize s.t. WH = data; always one iteration (sivm.py:203-228)."""
        self._check_supported()
        if compute_err and _is_sparse(self.data):
            raise TypeError("%s: compute_err=True on scipy.sparse data: the reference's frobenius_norm() only returns its "
                            "-123456 sentinel there; pass compute_err=False" % type(self).__name__)
        NMF.factorize(self, niter=1, show_progress=show_progress, compute_w=compute_w, compute_h=compute_h,
                      compute_err=compute_err)

    def _after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call=None):
        NMF._after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call)
        if compute_w and result[1] > 0:
            self._take_select(ctx)
