"""pymf_amd.GREEDYCUR -- drop-in for pymf.GREEDYCUR (reference pymf/greedycur.py) on MI355X, dense data.

A CUR decomposition whose rows and columns are chosen by GREEDY instead of drawn at random: `_cid` is GREEDY's selection on
the data, `_rid` GREEDY's selection on the transposed data, both with unit counts and in selection order (unsorted), and
computeUCR() is CUR's.  Both selections come from one float64 Gram matrix on the short side of the
data and its eigenpairs: the side with rows <= cols runs the pass over column panels, the other side runs in Gram space.
The `k` that the reference's sample() hands to GREEDY is ignored for dense data, as there.

As in CUR, `crank` follows `rrank`; rrank = 0 means all rows and all columns.

Supported: dense data, one rank, rrank <= 64, min(rows, cols) <= 2432.  scipy.sparse data raises TypeError, a multi-rank world
NotImplementedError, a larger rrank or short side ValueError.  When rrank exceeds the numerical rank of the data the later
selections are valid indices chosen as GREEDY's docstring describes.
"""
import numpy as np

from .cur import CUR
from .greedy import GREEDY, MAX_BASES, MAX_SHORT_SIDE

__all__ = ["GREEDYCUR"]


class GREEDYCUR(CUR):
    """
    GREEDYCUR(data, k=-1, rrank=0, crank=0)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> cur_mdl = GREEDYCUR(data, rrank=1, crank=2)
    >>> cur_mdl.factorize()
    """
    _TAKES_SPARSE = False     # no sparse device path: accept_sparse changes nothing here

    def _check_ranks(self):
        if self._rrank > MAX_BASES or self._crank > MAX_BASES:
            raise ValueError("GREEDYCUR: rrank > %d is not supported (rrank = 0 selects as many rows and columns as the data "
                             "have)" % MAX_BASES)
        if min(self._rows, self._cols) > MAX_SHORT_SIDE:
            raise ValueError("GREEDYCUR: min(rows, cols) > %d is not supported" % MAX_SHORT_SIDE)

    def sample(self, A, c):                                    # greedycur.py:62-68
        """GREEDY's selection of `c` columns of A, a list of Python ints in selection order.  A is the data or its transposed
        view (both run on the resident copy); any other matrix goes through a GREEDY object of its own."""
        self._check_supported()
        c = int(c)
        if c > MAX_BASES:
            raise ValueError("GREEDYCUR: more than %d selected rows or columns are not supported" % MAX_BASES)
        transposed = A is not self.data
        if transposed and not (isinstance(A, np.ndarray) and isinstance(self.data, np.ndarray) and A.ndim == 2
                               and A.shape == self.data.shape[::-1] and A.strides == self.data.strides[::-1]
                               and A.__array_interface__["data"][0] == self.data.__array_interface__["data"][0]):
            greedy_mdl = GREEDY(A, k=np.round(c - c / 5.0), num_bases=c)
            greedy_mdl.factorize(compute_h=False, compute_err=False, niter=1)
            return greedy_mdl.select
        if min(self._rows, self._cols) > MAX_SHORT_SIDE:
            raise ValueError("GREEDYCUR: min(rows, cols) > %d is not supported" % MAX_SHORT_SIDE)
        if not self._fresh:
            self._upload()
            self._fresh = True
        return [int(s) for s in self._context().greedy_select(c, transposed=transposed)]

    def factorize(self):                                       # greedycur.py:71-78
        self._check_supported()
        self._check_ranks()
        self._fresh = False
        self._rid = self.sample(self.data.transpose(), self._rrank)
        self._cid = self.sample(self.data, self._crank)
        self._rcnt = np.ones(len(self._rid))
        self._ccnt = np.ones(len(self._cid))

        self.computeUCR()
