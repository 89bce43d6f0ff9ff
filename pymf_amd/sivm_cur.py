"""pymf_amd.SIVM_CUR -- drop-in for pymf.SIVM_CUR (reference pymf/sivm_cur.py) on MI355X, dense data.

A CUR decomposition whose rows and columns are chosen by SIVM instead of drawn at random: `_cid` is SIVM's selection on the
data, `_rid` SIVM's selection on the transposed data, both with unit counts and in selection order (unsorted), and
computeUCR() is CUR's.  Both selections run on the one resident copy of the data: the columns through
SIVM's pass over column panels, the rows -- candidates as long as the data are wide -- through the long-sample pass, with no
transposed copy while rows <= 16384 (beyond that the two kernels change sides on a transposed copy).

Under the default init='origin' the first entry of `_rid` and `_cid` is -1, as in the reference (sivm.py:163-166);
computeUCR() reads it as a Python index, the LAST row or column, as the reference's indexing does.

As in CUR, `crank` follows `rrank`; rrank = 0 means all rows and all columns.

Supported: dense data, one rank, rrank <= 64, min(rows, cols) <= 16384, dist_measure 'l2', 'l1' or 'cosine'.  scipy.sparse data
raises TypeError, a multi-rank world NotImplementedError, a larger rrank or short side ValueError, the measures 'kl',
'abs_cosine' and 'weighted_abs_cosine' NotImplementedError, an unknown measure or init ValueError.
"""
import numpy as np

from .cur import CUR
from .sivm import SIVM, _INITS, _METRICS, _UNSUPPORTED_METRICS

__all__ = ["SIVM_CUR"]

MAX_BASES = 64           # pmf_sivm_select: nsel <= 64
MAX_SHORT_SIDE = 16384   # PMF_SIVM_MAX_M, PMF_SIVM_ROW_MAX_C (pmf_sivm.h)


class SIVM_CUR(CUR):
    """
    SIVM_CUR(data, k=-1, rrank=0, crank=0, dist_measure='l2', init='origin')

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> sivmcur_mdl = SIVM_CUR(data, rrank=1, crank=2)
    >>> sivmcur_mdl.factorize()
    """
    _TAKES_SPARSE = False     # no sparse device path: accept_sparse changes nothing here

    def __init__(self, data, k=-1, rrank=0, crank=0, dist_measure='l2', init='origin'):   # sivm_cur.py:60-63
        CUR.__init__(self, data, k=k, rrank=rrank, crank=rrank)
        self._dist_measure = dist_measure
        self.init = init

    def _check_supported(self):
        CUR._check_supported(self)
        if self._dist_measure in _UNSUPPORTED_METRICS:
            raise NotImplementedError("SIVM_CUR: dist_measure '%s' is not supported ('l2', 'l1' and 'cosine' are)" % self._dist_measure)
        if self._dist_measure not in _METRICS:
            raise ValueError("SIVM_CUR: unknown dist_measure %r" % (self._dist_measure,))
        if self.init not in _INITS:
            raise ValueError("SIVM_CUR: init must be 'fastmap' or 'origin', not %r" % (self.init,))

    def _check_ranks(self):
        if self._rrank > MAX_BASES or self._crank > MAX_BASES:
            raise ValueError("SIVM_CUR: rrank > %d is not supported (rrank = 0 selects as many rows and columns as the data "
                             "have)" % MAX_BASES)
        if min(self._rows, self._cols) > MAX_SHORT_SIDE:
            raise ValueError("SIVM_CUR: min(rows, cols) > %d is not supported" % MAX_SHORT_SIDE)

    def sample(self, A, c):                                    # sivm_cur.py:65-73
        """SIVM's selection of `c` columns of A, a list of Python ints in selection order.  A is the data or its transposed
        view (both run on the resident copy); any other matrix goes through a SIVM object of its own."""
        self._check_supported()
        c = int(c)
        if c > MAX_BASES:
            raise ValueError("SIVM_CUR: more than %d selected rows or columns are not supported" % MAX_BASES)
        transposed = A is not self.data
        if transposed and not (isinstance(A, np.ndarray) and isinstance(self.data, np.ndarray) and A.ndim == 2
                               and A.shape == self.data.shape[::-1] and A.strides == self.data.strides[::-1]
                               and A.__array_interface__["data"][0] == self.data.__array_interface__["data"][0]):
            sivm_mdl = SIVM(A, num_bases=c, dist_measure=self._dist_measure, init=self.init)
            sivm_mdl.factorize(show_progress=False, compute_w=True, niter=1, compute_h=False, compute_err=False)
            return sivm_mdl.select
        if min(self._rows, self._cols) > MAX_SHORT_SIDE:
            raise ValueError("SIVM_CUR: min(rows, cols) > %d is not supported" % MAX_SHORT_SIDE)
        if not self._fresh:
            self._upload()
            self._fresh = True
        sel = self._context().sivm_select(c, transposed=transposed, metric=_METRICS[self._dist_measure], init=_INITS[self.init])
        return [int(s) for s in sel]

    def factorize(self):                                       # sivm_cur.py:76-92
        self._check_supported()
        self._check_ranks()
        self._fresh = False
        self._rid = self.sample(self.data.transpose(), self._rrank)
        self._cid = self.sample(self.data, self._crank)
        self._rcnt = np.ones(len(self._rid))
        self._ccnt = np.ones(len(self._cid))

        self.computeUCR()
