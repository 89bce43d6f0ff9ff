"""pymf_amd.Kmeans -- drop-in for pymf.Kmeans (reference pymf/kmeans.py) on MI355X.

k-means as a factorization: W holds the centres, H is the one-hot assignment matrix, `assigned` the cluster index of every
sample.  One iteration is update_w (the mean of the members of every centre that has more than one, kmeans.py:82-87), then
update_h (assigned = argmin_j ||data[:, c] - W[:, j]||, the lowest index on ties, kmeans.py:75-79); on the device that is one
pass over the data per iteration, spread over column panels.  factorize()'s loop, error, convergence rule
and the truncation of `ferr` are NMF's (nmf.py:171-202).

The draw of the initial centres is the reference's: `random.sample(range(num_samples), num_bases)` on Python's global
`random` (kmeans.py:69), sorted, W = data[:, sel].

Supported: dense data of any shape, resident, one rank, num_bases <= 128.  scipy.sparse data raises TypeError, streamed data
(stream_rows) ValueError, a multi-rank world NotImplementedError, more than 128 bases ValueError.  update_w() before any
assignment exists (the caller set both W and H) raises AttributeError, as the reference's `self.assigned` would.

scipy.sparse data (opt-in: `mdl.accept_sparse = True`, the switch NMF, CUR, SVD and GREEDY have; Kmeans and Cmeans).  The
reference has no sparse clustering branch; what is computed is its dense rule on toarray().  The matrix is converted once to
canonical CSR (tocsr(), duplicates summed, indices sorted, float32 values, stored zeros kept; the caller's matrix is left
alone) and stays sparse on the device: the H step sweeps the samples' stored entries (k_cluster_csr_assign), the W step the
data rows' (k_cluster_csr_num); no dense image exists on host or device.  factorize(), update_w(), update_h(),
frobenius_norm(), init_w() and init_h() work; W is a dense ndarray (Kmeans.init_w binds data[:, sorted(sel)].toarray()), H a
dense float64 ndarray, `assigned` intp, ferr filled (compute_err=True works; NMF's -123456 sentinel is only returned without
factors).  ferr is sqrt(sum min d^2) right behind Kmeans' own H step and otherwise the float64 identity
||data||^2 - 2 <W^T data, H> + <W^T W, H H^T>, clamped at 0.  The other limits stay: resident, one rank, num_bases <= 128.
"""
import random

import numpy as np

from . import _lib
from .nmf import NMF, _is_sparse
from .svd import canonical_csr

__all__ = ["Kmeans"]


class _Clustering(NMF):
    """What Kmeans and Cmeans share: the refusals, and H rebound as a new float64 array by every H step (kmeans.py:78,
    cmeans.py:81) while W is updated in place (kmeans.py:87, cmeans.py:86)."""
    _MAX_BASES = 128
    accept_sparse = False     # opt-in, per object: scipy.sparse data stays sparse on the device (module docstring)

    def _sparse_run(self):
        """`data` is a scipy.sparse matrix and this object takes it (accept_sparse)."""
        return bool(self.accept_sparse) and _is_sparse(self.data)

    def _upload_sparse(self, ctx):
        self._check_supported()
        csr = canonical_csr(self.data)
        self._warn_if_float64(csr.data)
        ctx.set_v_csr(csr.indptr.astype(np.int64), csr.indices.astype(np.int32), csr.data.astype(np.float32))

    def _check_supported(self):
        name = type(self).__name__
        if _is_sparse(self.data) and not self._sparse_run():
            raise TypeError("%s: scipy.sparse data is not supported (dense data only)" % name)
        if self.stream_rows or self._stream_rows():
            raise ValueError("%s: streamed data (stream_rows) is not supported: the pass over column panels needs the data "
                             "resident" % name)
        if self._world().size > 1:
            raise NotImplementedError("%s: one rank only (a multi-rank world is not supported)" % name)
        if self._num_bases > self._MAX_BASES:
            raise ValueError("%s: num_bases > %d is not supported" % (name, self._MAX_BASES))

    def _download(self, ctx, name, cur):
        if name == "H":
            return ctx.get_h64()
        return NMF._download(self, ctx, name, cur)

    def update_w(self):
        self._check_supported()
        NMF.update_w(self)

    def update_h(self):
        self._check_supported()
        NMF.update_h(self)

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
        NMF.factorize(self, niter=niter, show_progress=show_progress, compute_w=compute_w, compute_h=compute_h,
                      compute_err=compute_err)


class Kmeans(_Clustering):
    _SHIPPED = True
    _ALGO = _lib.ALGO_KMEANS

    # ---- self.assigned: a plain attribute to the user; the device copy follows it -----------------------------------
    def _get_assigned(self):
        try:
            return self.__dict__["_assigned"]
        except KeyError:
            raise AttributeError("'%s' object has no attribute 'assigned'" % type(self).__name__)

    def _set_assigned(self, value):
        self.__dict__["_assigned"] = value
        self.__dict__["_assigned_on_device"] = False

    def _del_assigned(self):
        self._get_assigned()
        del self.__dict__["_assigned"]

    assigned = property(_get_assigned, _set_assigned, _del_assigned)

    def _take_assigned(self, ctx):
        self.__dict__["_assigned"] = ctx.get_assigned().astype(np.intp)     # np.argmin's dtype (dist.py:129)
        self.__dict__["_assigned_on_device"] = True

    def _sync_to_device_timed(self, ctx, with_data):
        ctx = NMF._sync_to_device_timed(self, ctx, with_data)
        if "_assigned" in self.__dict__ and not self.__dict__.get("_assigned_on_device", False):
            ctx.set_assigned(np.asarray(self.__dict__["_assigned"]).reshape(-1))
            self.__dict__["_assigned_on_device"] = True
        return ctx

    def __getstate__(self):
        st = NMF.__getstate__(self)
        st["_assigned_on_device"] = False
        return st

    # ---- the reference's hooks ------------------------------------------------------------------------------------
    def init_w(self):                                          # kmeans.py:67-72
        self._check_supported()
        sel = random.sample(range(self._num_samples), self._num_bases)
        if self._sparse_run():                                 # a dense W: the centres do not stay sparse
            self.W = np.asarray(self.data.tocsc()[:, np.sort(sel)].toarray())
        else:
            self.W = np.asarray(self.data[:, np.sort(sel)])

    def init_h(self):                                          # kmeans.py:62-65
        self.H = np.zeros((self._num_bases, self._num_samples))
        self._host_stale.add("H")                              # (about to be written on the device: the zeros do not go up)
        self.update_h()

    def update_h(self):                                        # kmeans.py:75-79
        self._check_supported()
        ctx = self._sync_to_device()
        ctx.update_h()
        self._take_assigned(ctx)
        self._pull(ctx, ("H",))

    def update_w(self):                                        # kmeans.py:82-87
        self._check_supported()
        self._get_assigned()                                   # AttributeError, as the reference's self.assigned
        NMF.update_w(self)

    def factorize(self, niter=1, show_progress=False, compute_w=True, compute_h=True, compute_err=True):
        """Factorize s.t. WH = data (nmf.py:141-202)."""
        self._check_supported()
        if not self._has("W"):                                 # nmf.py:173-177
            self.init_w()
        if not self._has("H"):
            self.init_h()
        if compute_w and niter > 0:
            self._get_assigned()                               # the loop's first update_w (nmf.py:183-184) reads self.assigned
        NMF.factorize(self, niter=niter, show_progress=show_progress, compute_w=compute_w, compute_h=compute_h,
                      compute_err=compute_err)

    def _after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call=None):
        NMF._after_device_loop(self, ctx, niter, result, compute_w, compute_h, compute_err, t_call)
        if compute_h and result[1] > 0:
            self._take_assigned(ctx)
