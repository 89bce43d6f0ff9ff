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
from .nmf import NMF, _fingerprint, _is_sparse

__all__ = ["CNMF"]


class CNMF(NMF):
    _SHIPPED = True
    _ALGO = _lib.ALGO_CNMF
    _REBIND_W = True                 # cnmf.py:175 rebinds self.W
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

    def _upload_sparse(self, ctx):
        raise TypeError("CNMF: scipy.sparse data is not supported (dense data only)")

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
                self.__dict__["_" + name] = np.zeros(shape)   # filled from the device when read
                self.__dict__["_%s_fp" % name.lower()] = None
                self._host_stale.add(name)

    # ---- host <-> device ---------------------------------------------------------------------------------
    def _sync_to_device_timed(self, ctx, with_data):
        if with_data and (not self._in_loop or not self._loop_data_checked):
            self._loop_data_checked = True
            self._upload_data(ctx)
        for name, setter in (("G", ctx.set_g), ("H", ctx.set_h), ("W", ctx.set_w)):
            if name in self._host_stale or not self._has(name):
                continue                                       # the device copy is the newer one / not there yet
            fp_attr = "_%s_fp" % name.lower()
            if (self.__dict__.get(fp_attr) is not None and name not in self._handed
                    and not self._held_elsewhere(name)):
                continue
            arr = self.__dict__["_" + name]
            if not np.issubdtype(np.asarray(arr).dtype, np.floating):
                raise TypeError("%s must be a floating-point array" % name)
            fp = _fingerprint(arr)
            if self.__dict__.get(fp_attr) != fp:
                self._uploaded = True
                setter(np.asarray(arr))
                self.__dict__[fp_attr] = fp
            del arr
            self._handed.discard(name)
        return ctx

    def _refresh_host(self, name):
        ctx = self._context()
        self._host_stale.discard(name)
        if name == "H":                                        # cnmf.py:167 rebinds H (float64, exact)
            self.__dict__["_H"] = ctx.get_h64()
        elif name == "W":                                      # cnmf.py:175 rebinds W = data G
            self.__dict__["_W"] = ctx.get_w().astype(np.float64)
        else:                                                  # cnmf.py:174 updates G in place
            cur = self.__dict__["_G"]
            np.copyto(cur, ctx.get_g(), casting="unsafe")
        self.__dict__["_%s_fp" % name.lower()] = _fingerprint(self.__dict__["_" + name])

    def _pull(self, ctx, want_w, want_h):
        NMF._pull(self, ctx, want_w, want_h)
        if want_w:
            self._host_stale.add("G")
            if not self._defer_pull and self._held_elsewhere("G"):
                self._refresh_host("G")

    def __getstate__(self):
        st = NMF.__getstate__(self)
        st["_g_fp"] = None
        return st

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
            self.__dict__["_W"] = np.zeros((self._data_dimension, self._num_bases))
            self.__dict__["_w_fp"] = None
            self._host_stale.add("W")
        self._tick("init", t_call)
        self.ferr = np.zeros(niter)                            # cnmf.py:154
        if self._hooks_overridden() or show_progress:
            return self._factorize_by_hooks(niter, compute_w, compute_h, compute_err)
        ctx = self._sync_to_device()
        ferr, done, conv_at = ctx.factorize(niter, compute_w, compute_h, compute_err, conv_eps=self._EPS)
        self._last_iters = done
        self._pull(ctx, compute_w and done > 0, compute_h and done > 0)
        self.last_call_ms["loop"] = ctx.last_loop_ms()
        self._tick("total", t_call)
        for i in range(done):
            if compute_err:
                self.ferr[i] = ferr[i]
                self._logger.info('Iteration ' + str(i + 1) + '/' + str(niter) + ' FN:' + str(self.ferr[i]))
            else:
                self._logger.info('Iteration ' + str(i + 1) + '/' + str(niter))
        if compute_err and conv_at >= 0:                       # cnmf.py:184-187
            self.ferr = self.ferr[:conv_at]

    def _factorize_by_hooks(self, niter, compute_w, compute_h, compute_err):
        """cnmf.py:156-187 one iteration per device call, with the (overridden) frobenius_norm / converged in between."""
        self._defer_pull = True
        self._in_loop = True
        self._loop_data_checked = False
        done = 0
        try:
            for i in range(niter):
                ctx = self._sync_to_device()
                ctx.factorize(1, compute_w, compute_h, False)
                self._pull(ctx, compute_w, compute_h)
                done = i + 1
                if compute_err:
                    self.ferr[i] = self.frobenius_norm()
                    self._logger.info('Iteration ' + str(i + 1) + '/' + str(niter) + ' FN:' + str(self.ferr[i]))
                else:
                    self._logger.info('Iteration ' + str(i + 1) + '/' + str(niter))
                if i > 1 and compute_err:
                    if self.converged(i):
                        self.ferr = self.ferr[:i]
                        break
        finally:
            self._defer_pull = False
            self._in_loop = False
            self._last_iters = done
            self._flush_host()
