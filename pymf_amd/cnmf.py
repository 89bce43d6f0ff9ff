"""pymf_amd.CNMF -- drop-in for pymf.CNMF (reference pymf/cnmf.py) on MI355X.

Convex NMF (Ding, Li, Jordan): W = data G with G >= 0 and H >= 0; data may be mixed-sign.  The reference initialises H and G
from k-means (pymf/kmeans.py, cnmf.py:78-103) and its factorize() runs every update on X^T X (cnmf.py:150-175).  Here the
whole loop and the k-means run on the device in Gram space: C = V^T V (n x n float64) is formed once per `data`, G and H
are kept in FLOAT64 on the device (a float64 self.G / self.H goes up and comes back exactly), and W = data G is written
when it is read, or once at the end of factorize() -- the W the reference holds at that point.

The draw of the initial centres is the reference's: `random.sample(range(num_samples), num_bases)` on Python's global
`random` (kmeans.py:71), so a seeded caller gets the reference's clusters.

Supported: dense data with num_samples <= 4096 and num_bases <= min(128, num_samples), one rank.  scipy.sparse data raises
TypeError, streamed data (stream_rows) ValueError, a multi-rank world NotImplementedError.  The hooks update_w / update_h /
init_w are no-ops as in the reference (cnmf.py:70-76,105-106); an overridden frobenius_norm or converged is called every
iteration.  One difference: an object given H and G but no W computes its error against data G where the reference's
frobenius_norm() would return its -123456 sentinel until a G step has set W.
"""
import logging
import random
import time

import numpy as np

from . import _lib
from .nmf import NMF, _is_sparse

__all__ = ["CNMF"]


class CNMF(NMF):
    _SHIPPED = True
    _ALGO = _lib.ALGO_CNMF
    _FACTORS = ("G", "H", "W")       # upload order
    _SKIP_MISSING_FACTORS = True     # init_h synchronises before H (and, unless the caller set them, G and W) exists
    _HOOKS = ("frobenius_norm", "converged")   # the reference's own loop calls no other hook (cnmf.py:156-187)
    _KMEANS_NITER = 10               # cnmf.py:86

    G = property(lambda self: self._factor_get("G"), lambda self, v: self._factor_set("G", v),
                 lambda self: self._factor_del("G"))

    # ---- refusals ----------------------------------------------------------------------------------
    def _check_supported(self):
        if _is_sparse(self.data):
            raise TypeError("CNMF: scipy.sparse data is not supported (dense data only)")
        if self.stream_rows or self._stream_rows():
            raise ValueError("CNMF: streamed data (stream_rows) is not supported: C = data^T data needs the data resident")
        if self._world().size > 1:
            raise NotImplementedError("CNMF: one rank only (a multi-rank world is not supported)")

    # ---- the reference's hooks -----------------------------------------------------------------------
    def update_w(self):                                        # cnmf.py:72-73
        pass

    def update_h(self):                                        # cnmf.py:75-76
        pass

    def init_w(self):                                          # cnmf.py:105-106
        pass

    def init_h(self):
        """cnmf.py:78-103: Kmeans(data, num_bases).factorize(niter=10) from random.sample'd centres, then H = onehot^T + 0.2,
        G = (onehot + 0.01) / count unless G exists, W = data G unless W exists -- all on the device."""
        if self._has("H"):
            return
        self._check_supported()
        k, n = self._num_bases, self._num_samples
        sel = np.sort(random.sample(range(n), k))              # kmeans.py:71-74
        ctx = self._sync_to_device()
        ctx.cnmf_init(sel, self._KMEANS_NITER)
        for name, shape in (("H", (k, n)), ("G", (n, k)), ("W", (self._data_dimension, k))):
            if name == "H" or not self._has(name):
                self._on_device_only(name, shape)

    def _on_device_only(self, name, shape):
        """A factor that exists on the device alone so far: its host array is filled when it is read."""
        self._factor_set(name, np.zeros(shape))
        self._host_stale.add(name)

    # ---- host <-> device ---------------------------------------------------------------------------------
    def _download(self, ctx, name, cur):
        if name == "H":                                        # cnmf.py:167 rebinds H (float64, exact)
            return ctx.get_h64()
        if name == "W":                                        # cnmf.py:175 rebinds W = data G
            return ctx.get_w().astype(np.float64)
        np.copyto(cur, ctx.get_g(), casting="unsafe")          # cnmf.py:174 updates G in place
        return cur

    def _moved(self, w_ran, h_ran):
        return NMF._moved(self, w_ran, h_ran) + (("G",) if w_ran else ())     # a W step is a G step: W = data G

    def frobenius_norm(self):
        """||data - W H|| (nmf.py:100-114): W = data G on the device, or the W the caller set."""
        self._check_supported()
        return NMF.frobenius_norm(self)

    # ---- factorize ------------------------------------------------------------------------------------------
    def factorize(self, niter=10, compute_w=True, compute_h=True, compute_err=True, show_progress=False):
        """Factorize s.t. WH = data (cnmf.py:108-187)."""
        self._logger.setLevel(logging.INFO if show_progress else logging.ERROR)
        self._check_supported()
        t_call = time.perf_counter()
        self.last_call_ms = {}
        if not self._has("W"):                                 # cnmf.py:133-134
            self.init_w()
        if not self._has("H"):                                 # cnmf.py:136-137
            self.init_h()
        if not self._has("G"):
            self.G                                             # AttributeError, as the reference's self.G (cnmf.py:159)
        if not self._has("W"):                                 # H and G given, no W: W = data G on the device
            self._on_device_only("W", (self._data_dimension, self._num_bases))
        self._tick("init", t_call)
        self.ferr = np.zeros(niter)                            # cnmf.py:154
        if self._hooks_overridden() or show_progress:
            return self._factorize_by_hooks(niter, compute_w, compute_h, compute_err)
        ctx = self._sync_to_device()
        result = ctx.factorize(niter, compute_w, compute_h, compute_err, conv_eps=self._EPS)
        self._after_device_loop(ctx, niter, result, compute_w, compute_h, compute_err, t_call)

    def _hook_iteration(self, compute_w, compute_h):
        """cnmf.py:156-175: one iteration per device call, the (overridden) frobenius_norm / converged run in between."""
        ctx = self._sync_to_device()
        ctx.factorize(1, compute_w, compute_h, False)
        self._pull(ctx, self._moved(compute_w, compute_h))
