"""pymf_amd.distance -- vq and pdist of the reference's distance module (pymf/dist.py:107-130) on MI355X.

    pdist(A, B, metric='l2')   the nA x nB float64 matrix of distances between the columns of A (d x nA) and of B (d x nB)
    vq(A, B, metric='l2')      np.argmin(pdist(A, B), axis=0) as intp: for every column of B the nearest column of A, the
                               lowest index among equally near ones

One side is the DATA: it lives on the device as a context's dense float32 V.  The other side, at most 128 columns, are the
QUERIES: they are measured against every data column in one sweep (pmf_vq_columns / pmf_vq_assign, pmf_vq.h).
With two arrays the side with more columns is the data (A on equal counts is the query side, as the reference loops) and is
uploaded to a context of its own for the call.  Either side may instead be a pymf_amd model (NMF, SIVM, AA, Kmeans ...): its
`data` is that side, its own context is used through `_sync_to_device()`, and nothing is uploaded when the data are already
resident -- `vq(mdl, mdl.W)` maps the bases of a fitted model onto data columns without the data leaving the device.

Arithmetic: float32 from the difference, `sqrt(sum((a - b)**2))` and `sum(abs(a - b))` as dist.py:61 and dist.py:33 form them
(no norm expansion), one running sum per pair; a distance is within (d + 4) 2^-24 of the float64 value on the float32-rounded
inputs, and the index is the reference's wherever the two nearest distances differ by more than twice that.  The result is
widened to float64.  float64 input is rounded to float32 and a PrecisionWarning says so, once per call.

Differences from the reference: a metric other than 'l2' or 'l1' raises ValueError (the reference silently returns a matrix of
zeros, and vq then index 0 everywhere); more than 128 columns on both sides raises ValueError; scipy.sparse input raises
TypeError (the reference's sparse branch of l2_distance is not built here); a model whose data are sparse or streamed raises
ValueError; distances that are NaN never win (np.argmin would return the first NaN).
"""
import sys
import warnings

import numpy as np

from . import _lib
from .nmf import PrecisionWarning

__all__ = ["vq", "pdist"]

MAX_QUERIES = 128                                    # PMF_VQ_MAX_Q
_METRICS = {"l2": 0, "l1": 1}


def _is_sparse(x):
    sp = sys.modules.get("scipy.sparse")
    return sp is not None and sp.issparse(x)


def _is_model(x):
    return hasattr(x, "_sync_to_device") and hasattr(x, "data")


def _metric(metric):
    try:
        return _METRICS[metric]
    except (KeyError, TypeError):
        raise ValueError("metric must be 'l2' or 'l1', not %r (the reference returns zeros for any other name)" % (metric,))


class _Side(object):
    """One operand: a model (its data are the columns, its context the device copy) or an array."""

    def __init__(self, x, name):
        self.model = x if _is_model(x) else None
        src = x.data if self.model is not None else x
        if _is_sparse(src):
            if self.model is not None:
                raise ValueError("vq / pdist: the data of %s %s are scipy.sparse; dense resident data only" % (name, type(x).__name__))
            raise TypeError("vq / pdist: scipy.sparse input is not supported (%s)" % name)
        if self.model is not None:
            self.arr = None
            self.shape = tuple(int(s) for s in src.shape)
            self.f64 = getattr(src, "dtype", None) == np.float64
        else:
            self.arr = np.asarray(src)
            if self.arr.ndim != 2:
                raise ValueError("vq / pdist: %s must be a d x n array" % name)
            self.shape = self.arr.shape
            self.f64 = self.arr.dtype == np.float64      # (a list of Python floats is float64 too; integers convert exactly)

    def host(self):
        """The columns as a host array (a query side)."""
        return self.arr if self.model is None else np.asarray(self.model.data[:, :])


def _model_context(mdl):
    """The model's own context with its data resident.  A fitted model goes through `_sync_to_device()` (data and factors, as
    before any of its steps); one whose factors are not set yet needs its data only: `_sync_to_device()` would raise the
    AttributeError of a missing W there."""
    if mdl._SKIP_MISSING_FACTORS or all(mdl._has(f) for f in mdl._FACTORS):
        return mdl._sync_to_device()
    ctx = mdl._context()
    mdl._upload_data(ctx)
    return ctx


def _plan(A, B):
    """(queries float32 d x nq, context, owned, data_is_a): which side is the data, and its context with the data resident."""
    a, b = _Side(A, "A"), _Side(B, "B")
    if a.shape[0] != b.shape[0]:
        raise ValueError("vq / pdist: A is %d x %d, B is %d x %d: the dimensions differ" % (a.shape + b.shape))
    na, nb = a.shape[1], b.shape[1]
    if a.model is not None and b.model is None:
        data_is_a = True
    elif b.model is not None and a.model is None:
        data_is_a = False
    else:
        data_is_a = na > nb                          # dist.py:111: A is looped over (the query side) while nA <= nB
    data, qry = (a, b) if data_is_a else (b, a)
    if qry.shape[1] > MAX_QUERIES:
        if data.shape[1] <= MAX_QUERIES:             # (a model with few samples against many columns: it is the query side)
            data, qry, data_is_a = qry, data, not data_is_a
        else:
            raise ValueError("vq / pdist: one side must have at most %d columns (A has %d, B has %d)" % (MAX_QUERIES, na, nb))
    if qry.shape[1] < 1 or data.shape[1] < 1 or a.shape[0] < 1:
        raise ValueError("vq / pdist: empty operand")
    if (a.f64 or b.f64):
        warnings.warn("vq / pdist: float64 input is rounded to float32 on the device (fp32 arithmetic from the difference; "
                      "the reference would compute in float64, dist.py:33,61)", PrecisionWarning, stacklevel=3)     # (_plan, vq / pdist, the caller)
    Q = np.ascontiguousarray(qry.host(), dtype=np.float32)
    if data.model is not None:
        mdl = data.model
        if getattr(mdl, "_stream_rows", lambda: 0)():
            raise ValueError("vq / pdist: the data of %s are streamed; dense resident data only" % type(mdl).__name__)
        return Q, _model_context(mdl), False, data_is_a
    ctx = _lib.Context(_lib.ALGO_CUR, data.shape[0], data.shape[1], 1)     # (the family without a limit on the shape)
    try:
        ctx.set_v_dense(data.arr)
    except BaseException:
        ctx.close()
        raise
    return Q, ctx, True, data_is_a


def pdist(A, B, metric='l2'):
    """The nA x nB float64 matrix of `metric` distances between the columns of A and of B (pymf/dist.py:107-124)."""
    met = _metric(metric)
    Q, ctx, owned, data_is_a = _plan(A, B)
    try:
        _, d = ctx.vq_assign(Q, met, want_idx=False, want_dist=True)       # [queries][data columns]
    finally:
        if owned:
            ctx.close()
    return np.ascontiguousarray(d.T) if data_is_a else d


def vq(A, B, metric='l2'):
    """For every column of B the index of the nearest column of A, intp (pymf/dist.py:126-130)."""
    met = _metric(metric)
    Q, ctx, owned, data_is_a = _plan(A, B)
    try:
        if data_is_a:
            idx, _ = ctx.vq_columns(Q, met, want_dist=False)               # per query (a column of B) the nearest data column
        else:
            idx, _ = ctx.vq_assign(Q, met, want_idx=True, want_dist=False)  # per data column (of B) the nearest query
    finally:
        if owned:
            ctx.close()
    return idx.astype(np.intp)
