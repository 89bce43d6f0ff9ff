"""pymf_amd.GMAP -- drop-in for pymf.GMAP (reference pymf/gmap.py) with robust_map=False on MI355X.

Geometric map: the first column is the one of largest norm ('pca', 'aa') or the one furthest in angle from the all-ones
direction ('nmf'); every further round multiplies a per-column volume estimate `iterval` by a factor formed from the cosine c
between the column and the last selected one -- (1 - |c|) |v| ('pca'), ((1 - c) / 2) |v| ('aa'), 1 - |c| ('nmf') -- and
selects its argmax (gmap.py:119-165).  H and ferr are AA's, as for SIVM.  On the device update_w is num_bases launches of
k_gmap_pass enqueued back to back on a SIVM context under the option sivm_rule = 2: sums of squares and dot
products in fp32, norms, cosines and iterval in float64.

Differences from the reference, both deliberate:
  * robust_map=True (the constructor's default, kept for signature parity) raises NotImplementedError from factorize,
    update_w, update_h and frobenius_norm: pass robust_map=False.  The reference's robust path cannot run on a current NumPy
    (robust_nselect = np.round(...) is a float used as a slice bound: TypeError) and depends on random.sample inside a nested
    Kmeans, so there is nothing to be equal to.
  * a zero-norm column makes c = 0 / 0 = NaN; here a NaN never wins the argmax, the reference's np.argmax would pick it.
A `method` other than 'pca', 'aa' or 'nmf' raises ValueError (the reference fails on an undefined `iterval`).

`select`, W, H, factorize()'s single iteration and the limits are SIVM's: dense resident data, one rank, num_bases <= 64,
data_dimension <= 16384.  `sub` stays empty (the robust path fills it in the reference).
"""
from .nmf import NMF
from .sivm import SIVM

__all__ = ["GMAP"]

_METHODS = {"pca": 0, "aa": 1, "nmf": 2}


class GMAP(SIVM):
    """
    GMAP(data, num_bases=4, method='pca', robust_map=True)

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> gmap_mdl = GMAP(data, num_bases=2, robust_map=False)
    >>> gmap_mdl.factorize()

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5, 1.3], [1.2, 0.3]])
    >>> gmap_mdl = GMAP(data, num_bases=2, robust_map=False)
    >>> gmap_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> gmap_mdl.factorize(compute_w=False)
    """
    _TAKES_SPARSE = False                                      # (SIVM's and LAESA's rule alone run on CSC data: DESIGN.md 3.23)

    def __init__(self, data, num_bases=4, method='pca', robust_map=True):
        SIVM.__init__(self, data, num_bases=num_bases)
        self.sub = []
        self._robust_map = robust_map
        self._method = method

    def _check_supported(self):
        SIVM._check_supported(self)
        if self._method not in _METHODS:
            raise ValueError("GMAP: method must be 'pca', 'aa' or 'nmf', not %r" % (self._method,))
        if self._robust_map:
            raise NotImplementedError("GMAP: robust_map=True is not supported (the reference's robust path depends on a randomly "
                                      "initialised nested Kmeans); pass robust_map=False")

    def _context(self):
        fresh = self._ctx is None
        ctx = SIVM._context(self)
        if fresh:
            ctx.set_option("sivm_rule", 2)
            ctx.set_option("gmap_method", _METHODS[self._method])
        return ctx

    def factorize(self, show_progress=False, compute_w=True, compute_h=True, compute_err=True, robust_cluster=3, niter=1,
                  robust_nselect=-1):
        """Factorize s.t. WH = data; always one iteration (gmap.py:175-215).  robust_cluster and robust_nselect belong to the
        robust path and are not used."""
        self._check_supported()
        NMF.factorize(self, niter=1, show_progress=show_progress, compute_w=compute_w, compute_h=compute_h,
                      compute_err=compute_err)
