"""pymf_amd.CMD -- drop-in for pymf.CMD (reference pymf/cmd.py) on MI355X, dense data.

Compact matrix decomposition: CUR's sampling, then repeated row and column indices are merged and carried as
multiplicities (`_rcnt`, `_ccnt`; cmd.py:56-70), which scale the kept rows and columns by their square roots in
CUR.computeUCR.  Device path and limits are CUR's (pymf_amd/cur.py).
"""
import numpy as np

from .cur import CUR

__all__ = ["CMD"]


class CMD(CUR):
    """
    CMD(data, k=-1, rrank=0, crank=0)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> cmd_mdl = CMD(data, rrank=1, crank=2)
    >>> cmd_mdl.factorize()
    """

    def _cmdinit(self):                                        # cmd.py:56-70
        nrids = np.unique(self._rid)
        ncids = np.unique(self._cid)

        self._rcnt = np.zeros(len(nrids))
        self._ccnt = np.zeros(len(ncids))

        for i, idx in enumerate(nrids):
            self._rcnt[i] = len(np.where(self._rid == idx)[0])

        for i, idx in enumerate(ncids):
            self._ccnt[i] = len(np.where(self._cid == idx)[0])

        self._rid = np.int32(list(nrids))
        self._cid = np.int32(list(ncids))

    def factorize(self):                                       # cmd.py:72-89
        self._check_supported()
        self._check_ranks()
        [prow, pcol] = self.sample_probability()

        self._rid = self.sample(self._rrank, prow)
        self._cid = self.sample(self._crank, pcol)

        self._cmdinit()

        self.computeUCR()
