"""pymf_amd.SIVM_GSAT -- drop-in for pymf.SIVM_GSAT (reference pymf/sivm_gsat.py) on MI355X.

The online member of the SIVM family, and the only one that improves a selection it is given: the simplex starts from the
first num_bases data columns (init_w; or from any W and `select` the caller sets, e.g. SIVM_SGREEDY's), and every probe -- a
randomly drawn data column (update_w) or any vector (online_update_w) -- replaces the vertex whose replacement gives the largest
Cayley-Menger volume, if that is at least the current volume V (sivm_gsat.py:82-125).  Rejected probes change nothing, so the
device evaluates probes 256 to a launch against the current simplex, applies the first accepted one and evaluates the probes
behind it again: the reference's sequence, decision for decision.  Distances and volumes are float64, formed
from the float32 values of the data and of W.

factorize(niter=N) runs N probes.  With compute_h=False and compute_err=False the N indices are drawn at once
(np.random.random(N): the stream a seeded caller sees is that of N single draws) and walked in ONE library call; otherwise
every iteration is one probe, SIVM's H step and the error, without a convergence test, as in the reference.  `select` is a
list, edited in place; W is edited in place; V is the current volume; `_v` appears with the first swap as [the volume before
it, every accepted volume ...]; D reads as the reference leaves it: (num_bases + 1) x (num_bases + 1) float64, the l2
distances among the vertices and, in its last row and column, the distances of the last probe that was evaluated.
dist_measure 'l2' or 'l1' applies to the distances between a probe and the vertices only: the distances among the vertices
stay l2, exactly as the reference mixes them.  'cosine' raises NotImplementedError: the reference's cosine_distance cannot
take the num_bases columns of W (dist.py:73-82 broadcasts them against each other).

Decisions are the reference's while num_bases <= data_dimension + 1 on data in general position.  Beyond that every volume
is rounding noise in the reference too; the walk then still returns valid slots and in-range indices.  A W or `select` that
the caller replaces between two probes starts the walk's state again from them (D and V from W alone, where the reference
would go on with the D it has until the next swap).

Limits are SIVM's: dense resident data, one rank, num_bases <= 64, data_dimension <= 16384.
"""
import logging

import numpy as np

from .nmf import NMF
from .sivm import SIVM

__all__ = ["SIVM_GSAT"]


class SIVM_GSAT(SIVM):
    """
    SIVM_GSAT(data, num_bases=4, dist_measure='l2', init='fastmap')

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> sivm_mdl = SIVM_GSAT(data, num_bases=2)
    >>> sivm_mdl.factorize()

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5, 1.3], [1.2, 0.3]])
    >>> sivm_mdl = SIVM_GSAT(data, num_bases=2)
    >>> sivm_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> sivm_mdl.factorize(compute_w=False)
    """
    _SHIPPED = True
    _NITER = None                                              # any number of iterations (sivm_gsat.py:168)
    _TAKES_SPARSE = False                                      # (SIVM's and LAESA's rule alone run on CSC data: DESIGN.md 3.23)

    def _check_supported(self):
        SIVM._check_supported(self)
        if self._dist_measure == "cosine":
            raise NotImplementedError("SIVM_GSAT: dist_measure 'cosine' is not supported ('l2' and 'l1' are): the reference's "
                                      "cosine_distance cannot take the num_bases columns of W")

    def _context(self):
        fresh = self._ctx is None
        ctx = SIVM._context(self)
        if fresh:
            ctx.set_option("sivm_gsat", 1)
        return ctx

    def _download(self, ctx, name, cur):
        if name == "W":                                        # sivm_gsat.py:106 writes the column into the W at hand
            return NMF._download(self, ctx, name, cur)
        return SIVM._download(self, ctx, name, cur)

    # ---- the walk's state on the device ---------------------------------------------------------------------------
    def _select_now(self):
        """`select` as the device takes it; a model without one (online_update_w on a caller's W) names no data column"""
        if "select" not in self.__dict__:
            return [-1] * self._num_bases
        return [int(s) for s in self.select]

    def _gsat_ready(self):
        """The context with data and W current and the walk's state belonging to them"""
        self._check_supported()
        ctx = self._sync_to_device()
        sel = self._select_now()
        if ctx.gsat_start(sel, force=sel != self.__dict__.get("_gs_select")):
            self._gs_select = sel
            self._gs_v_before = list(self._v) if "_v" in self.__dict__ else None
            self.V = ctx.gsat_get_volumes()[1]                 # sivm_gsat.py:88
        return ctx

    def _after_probes(self, ctx, swapped):
        if not swapped:
            return
        log, V = ctx.gsat_get_volumes()
        before = self._gs_v_before
        self._v = [float(v) for v in log] if before is None else before + [float(v) for v in log[1:]]
        self.V = V
        self._pull(ctx, ("W",))

    def _walk(self, idx):
        """The probes idx (data columns) in order; the slot each replaced, -1 rejected, -2 skipped"""
        ctx = self._gsat_ready()
        slots = ctx.gsat_walk(idx)
        self._last_slots = slots
        for n, s in zip(idx, slots):
            if s >= 0:
                self.select[int(s)] = int(n)                   # sivm_gsat.py:124
                self._logger.info('Current selection:' + str(self.select))
        self._gs_select = self._select_now()
        self._after_probes(ctx, bool((slots >= 0).any()))
        return slots

    @property
    def D(self):
        if self._ctx is None or "_gs_select" not in self.__dict__:
            raise AttributeError("'%s' object has no attribute 'D'" % type(self).__name__)   # (no probe yet: sivm_gsat.py:85)
        return self._gsat_ready().gsat_get_d()

    # ---- the reference's hooks ------------------------------------------------------------------------------------
    def init_w(self):                                          # sivm_gsat.py:78-80 (a list: select[s] = n must work)
        self.select = list(range(self._num_bases))
        self.W = np.array(self.data[:, self.select])

    def online_update_w(self, vec):                            # sivm_gsat.py:82-117
        ctx = self._gsat_ready()
        s = ctx.gsat_probe_vec(np.asarray(vec).reshape(-1))
        self._after_probes(ctx, s >= 0)
        if s >= 0:
            self._logger.info('Volume increased:' + str(self.V))
            return True, s
        return False, -1

    def _draw(self, count=None):                               # sivm_gsat.py:120
        return np.floor(np.random.random(count) * self._num_samples).astype(np.int64)

    def update_w(self):                                        # sivm_gsat.py:119-125
        self._walk(self._draw(1))

    def converged(self, i):                                    # (no convergence test: sivm_gsat.py:168-180)
        return False

    def factorize(self, show_progress=False, compute_w=True, compute_h=True, compute_err=True, niter=1):
        """Factorize s.t. WH = data; niter probes (sivm_gsat.py:128-180)."""
        self._check_supported()
        self._logger.setLevel(logging.INFO if show_progress else logging.ERROR)
        self.last_call_ms = {}
        if not self._has('W'):
            self.init_w()
        if not self._has('H'):
            self.init_h()
        if compute_err:
            self.ferr = np.zeros(niter)
        if compute_h or compute_err or show_progress or self._hooks_overridden():
            return self._factorize_by_hooks(niter, compute_w, compute_h, compute_err)
        if compute_w and niter > 0:
            self._walk(self._draw(niter))
        for i in range(niter):
            self._log_iteration(i, niter)
