"""pymf_amd.CHNMF -- drop-in for pymf.CHNMF (reference pymf/chnmf.py) on MI355X.

Convex-hull NMF: the data are projected onto base_sel random directions, proj = R data (chnmf.py:180-181); for every pair of
projected coordinates the vertices of the 2-D convex hull are found (quickhull, chnmf.py:27-60), mapped back to sample indices
(the first index among duplicates) and collected in `_hull_idx`, ascending (chnmf.py:154-170).  W is then archetypal analysis
of those few columns alone, 50 iterations (chnmf.py:184-190); H and ferr are AA's on the full data.  `Wmapped` /
`_Wmapped_index` hold the data column nearest to each base (chnmf.py:137-150); W itself stays AA's.

On the device: R is drawn on the host -- one np.random.randn(base_sel, data_dimension) call, the first thing
update_w does, as in the reference --, proj is formed in float64 on the float64 MFMA and stays on the device, and every pair's
hull is a filter sweep over all samples followed by an exact monotone chain over the survivors, all pairs enqueued back to
back (pmf_chnmf_hull).  Every comparison that decides hull membership is float64.  The hull points are vertices in the strict
sense of the reference's `dists > 0`; on data in general position `_hull_idx` is the reference's exactly.  The nested AA runs
through pymf_amd.AA on data[:, _hull_idx] (a host gather: the subset is small); _map_w_to_data runs on the host in float64.

Supported: dense resident data, one rank, 2 <= base_sel <= 16 (after the reference's clipping to data_dimension), and AA's
limits on both the full data and the subset (num_bases <= 64, min(data_dimension + 1, num_samples) <= 128).  scipy.sparse data
raises TypeError, streamed data ValueError, a multi-rank world NotImplementedError, a base_sel outside the range ValueError.
"""
import logging

import numpy as np

from .aa import AA
from .nmf import NMF

__all__ = ["CHNMF"]


class CHNMF(AA):
    """
    CHNMF(data, num_bases=4, base_sel=3)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> chnmf_mdl = CHNMF(data, num_bases=2)
    >>> chnmf_mdl.factorize()

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5, 2.0], [1.2, 1.8]])
    >>> chnmf_mdl = CHNMF(data, num_bases=2)
    >>> chnmf_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> chnmf_mdl.factorize(compute_w=False)
    """
    _SHIPPED = True
    _SKIP_MISSING_FACTORS = True                               # update_w needs neither factor (it rebinds W), update_h no H
    _MAX_BASE_SEL = 16
    _NITER_AA = 50                                             # chnmf.py:187

    def __init__(self, data, num_bases=4, base_sel=3):
        super(CHNMF, self).__init__(data, num_bases=num_bases)
        self._base_sel = base_sel                              # chnmf.py:127-129: never larger than the data dimension
        if base_sel > self.data.shape[0]:
            self._base_sel = self.data.shape[0]

    def _check_supported(self):
        super(CHNMF, self)._check_supported()
        if not 2 <= self._base_sel <= self._MAX_BASE_SEL:
            raise ValueError("CHNMF: base_sel (after clipping to data_dimension) must be 2 .. %d, not %r"
                             % (self._MAX_BASE_SEL, self._base_sel))

    # ---- the reference's hooks ------------------------------------------------------------------------------------
    def init_h(self):                                          # chnmf.py:131-132
        self.H = np.zeros((self._num_bases, self._num_samples))

    def init_w(self):                                          # chnmf.py:134-135
        self.W = np.zeros((self._data_dimension, self._num_bases))

    def _map_w_to_data(self):                                  # chnmf.py:137-150: vq = argmin of the l2 distances, first index wins
        W = np.asarray(self.W, dtype=np.float64)
        best = np.full(self._num_bases, np.inf)
        self._Wmapped_index = np.zeros(self._num_bases, dtype=np.int64)
        step = max(1, (1 << 22) // max(self._data_dimension, 1))
        for c0 in range(0, self._num_samples, step):
            blk = np.asarray(self.data[:, c0:c0 + step], dtype=np.float64)
            for i in range(self._num_bases):
                d = ((blk - W[:, i:i + 1]) ** 2).sum(axis=0)
                j = int(np.argmin(d))
                if d[j] < best[i]:                             # (strictly: an earlier block keeps a tie)
                    best[i], self._Wmapped_index[i] = d[j], c0 + j
        self.Wmapped = np.zeros(self.W.shape)
        for i, s in enumerate(self._Wmapped_index):
            self.Wmapped[:, i] = self.data[:, s]

    def update_w(self):                                        # chnmf.py:152-191
        self._check_supported()
        R = np.random.randn(self._base_sel, self._data_dimension)   # chnmf.py:180: the first draw of the step
        ctx = self._sync_to_device()
        self._hull_idx = ctx.chnmf_hull(R)                     # select_hull_points(R data), int32 ascending
        aa_mdl = AA(np.ascontiguousarray(self.data[:, self._hull_idx]), num_bases=self._num_bases)
        aa_mdl.factorize(niter=self._NITER_AA, compute_h=True, compute_w=True, compute_err=True, show_progress=False)
        self._aa_ferr = aa_mdl.ferr
        self.W = aa_mdl.W                                      # chnmf.py:190 rebinds W
        self._map_w_to_data()

    def factorize(self, show_progress=False, compute_w=True, compute_h=True, compute_err=True, niter=1):
        """Factorize s.t. WH = data; always one iteration (chnmf.py:193-218)."""
        self._check_supported()
        self._logger.setLevel(logging.INFO if show_progress else logging.ERROR)   # nmf.py:166-169
        self.last_call_ms = {}
        if not self._has('W'):                                 # nmf.py:173-177
            self.init_w()
        if not self._has('H'):
            self.init_h()
        if compute_err:
            self.ferr = np.zeros(1)
        # update_w is a host composition (projection draw, device hull pass, nested AA): the hook loop of nmf.py:182-202
        NMF._factorize_by_hooks(self, 1, compute_w, compute_h, compute_err)
