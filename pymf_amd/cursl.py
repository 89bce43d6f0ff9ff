"""pymf_amd.CURSL -- drop-in for pymf.CURSL (reference pymf/cursl.py) on MI355X, dense data.

CURSL is CMD with the sampling probabilities replaced by statistical leverage scores (Drineas, Kannan and Mahoney): a
column is drawn with a probability proportional to its squared norm in the leading k right singular vectors of the data, a
row with its squared norm in the leading k left singular vectors (cursl.py:65-91; `comp_prob` takes the full dense SVD, the
`k` it hands to SVD is ignored for dense data, and `V[:k]` is the leading min(k, rank) vectors above svd.py's 1e-8 cut).
The column probabilities use k = `_rrank`, the row probabilities k = `_crank`, as the reference does; they differ only for
`rrank = 0`.

On the device both come from the eigenpairs of the float64 Gram matrix on the short side of the data (the float64 Jacobi,
cached per upload): the eigenvector side directly, the long side by one read of the float32 data on the float64 MFMA
(k_lev_f64) -- the reference's `V = S^-1 U^T data`, 512 MB at 64 x 1 048 576, is never written.  The draws,
CMD's merge of repeated indices and computeUCR are inherited (pymf_amd/cmd.py, pymf_amd/cur.py).

Supported: CUR's limits (dense data, one rank, rrank <= 128; rrank = 0 needs data that small) and min(rows, cols) <= 2432.
"""
from .cmd import CMD
from .cur import CUR

__all__ = ["CURSL"]

MAX_SHORT_SIDE = 2432      # PMF_SVD_MAX_RANK (pmf_svd.h)


class CURSL(CMD):
    """
    CURSL(data, k=-1, rrank=0, crank=0)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> cur_mdl = CURSL(data, rrank=1, crank=2)
    >>> cur_mdl.factorize()
    """
    _TAKES_SPARSE = False     # no sparse device path: accept_sparse changes nothing here

    def __init__(self, data, k=-1, rrank=0, crank=0):          # cursl.py:62-63
        CUR.__init__(self, data, k=k, rrank=rrank, crank=crank)

    def _check_ranks(self):
        CMD._check_ranks(self)
        if min(self._rows, self._cols) > MAX_SHORT_SIDE:
            raise ValueError("CURSL: min(rows, cols) > %d is not supported" % MAX_SHORT_SIDE)

    def sample_probability(self):                              # cursl.py:65-91
        self._check_supported()
        self._check_ranks()
        ctx = self._upload()
        self._fresh = True
        prow, pcol = ctx.cur_leverage(self._crank, self._rrank)
        pcol /= self._rrank                                    # comp_prob(data, _rrank): A.sum(axis=0) / k, then normalised
        pcol /= pcol.sum()
        prow /= self._crank                                    # comp_prob(data.T, _crank)
        prow /= prow.sum()
        return (prow.reshape(-1, 1), pcol.reshape(-1, 1))
