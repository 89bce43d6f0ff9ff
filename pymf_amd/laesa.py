"""pymf_amd.LAESA -- drop-in for pymf.LAESA (reference pymf/laesa.py) on MI355X.

Maximin column selection: after SIVM's start (init_sivm, sivm.py:145-166: three distance passes for 'fastmap', one for
'origin') every round keeps, per column, the smallest distance to any column selected so far and selects the column where
that minimum is largest (laesa.py:63-82).  H and ferr are AA's, as for SIVM.  On the device update_w is num_bases + 2
('fastmap') or num_bases ('origin') launches of k_laesa_pass enqueued back to back on a SIVM context under the option
sivm_rule = 1: distances in fp32, the running minimum in float64.  The reference measures against
select[0] twice and takes the minimum of the two equal vectors; the device runs that pass once.

Everything else is SIVM's: the constructor, `select` in selection order with -1 first under init='origin' (that column of W
is the LAST data column), W as data columns in the data's dtype, the float64 H, one iteration per factorize(), and the
limits -- dense resident data (scipy.sparse data raises TypeError here, as before; the device pass for LAESA's rule on CSC data
exists and is reached through the C ABI: DESIGN.md 3.23), one rank, num_bases <= 64, data_dimension <= 16384, dist_measure 'l2', 'l1' or 'cosine'.
"""
from .sivm import SIVM

__all__ = ["LAESA"]


class LAESA(SIVM):
    """
    LAESA(data, num_bases=4, dist_measure='l2', init='fastmap')

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> laesa_mdl = LAESA(data, num_bases=2)
    >>> laesa_mdl.factorize()

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5, 1.3], [1.2, 0.3]])
    >>> laesa_mdl = LAESA(data, num_bases=2)
    >>> laesa_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> laesa_mdl.factorize(niter=1, compute_w=False)
    """
    _TAKES_SPARSE = False                                      # (the class keeps its refusal)

    def _context(self):
        fresh = self._ctx is None
        ctx = SIVM._context(self)
        if fresh:
            ctx.set_option("sivm_rule", 1)
        return ctx
