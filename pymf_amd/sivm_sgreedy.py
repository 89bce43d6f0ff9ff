"""pymf_amd.SIVM_SGREEDY -- drop-in for pymf.SIVM_SGREEDY (reference pymf/sivm_sgreedy.py) on MI355X.

The exact member of the SIVM family: after SIVM's start (init_sivm, sivm.py:145-166: three distance passes for 'fastmap', one
for 'origin', of which only select[0] is kept) every round evaluates, for EVERY column, the Cayley-Menger volume of "columns
selected so far + that column" from pairwise l2 distances (vol.py:24-34) and selects the argmax (sivm_sgreedy.py:96-133).  The
reference forms one determinant per column per round; the device forms det(CM_S) (-b^T inv(CM_S) b) with inv(CM_S) and
det(CM_S) shared by all columns: num_bases - 1 rounds of k_sgreedy_step and k_sgreedy_pass on a SIVM context
under the option sivm_sgreedy = 1, squared distances in fp32, everything behind them in float64, no host read in between.

`select` is in the reference's order: its first num_bases - 1 picks sorted ascending, then the last pick; under init='origin'
the first entry is -1 (a Python index: that column of W, the first vertex, is the LAST data column).  W holds those data
columns in the data's dtype.  `_v` lists the num_bases - 1 winning volumes as float64.  `_t` lists num_bases - 1 floats as the
reference does, but the rounds are not synchronised with the host, so every entry repeats the elapsed time of the whole
update_w call.  num_bases = 1 runs no round: `_v` and `_t` are empty.  dist_measure applies to the start only; the volumes are
always l2, as in the reference.  The constructor is SIVM's (the niter / compW arguments of the reference's docstring do not
exist in its code).  H, ferr and factorize() are SIVM's, which are AA's.

Selections are the reference's while the selected columns stay affinely independent: num_bases <= data_dimension + 1 on data
in general position.  Beyond that every volume is rounding noise in the reference too; update_w then still returns valid,
in-range indices (possibly repeated), and update_h raises as for SIVM, because W^T W is singular.

Limits are SIVM's: dense resident data, one rank, num_bases <= 64, data_dimension <= 16384, dist_measure 'l2', 'l1' or 'cosine'.
"""
import time

from .sivm import SIVM

__all__ = ["SIVM_SGREEDY"]


def reference_order(picks):
    """The reference's `select` from the picks in selection order: next_sel is re-sorted at the top of every round and the last
    pick is appended behind the last sort (sivm_sgreedy.py:106-132)."""
    picks = [int(s) for s in picks]
    return sorted(picks[:-1]) + picks[-1:]


class SIVM_SGREEDY(SIVM):
    """
    SIVM_SGREEDY(data, num_bases=4, dist_measure='l2', init='fastmap')

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> sivm_mdl = SIVM_SGREEDY(data, num_bases=2)
    >>> sivm_mdl.factorize()

    Coefficients for an existing set of basis vectors: set W and pass compute_w=False.

    >>> data = np.array([[1.5, 1.3], [1.2, 0.3]])
    >>> sivm_mdl = SIVM_SGREEDY(data, num_bases=2)
    >>> sivm_mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    >>> sivm_mdl.factorize(compute_w=False)
    """
    _TAKES_SPARSE = False                                      # (SIVM's and LAESA's rule alone run on CSC data: DESIGN.md 3.23)

    def _context(self):
        fresh = self._ctx is None
        ctx = SIVM._context(self)
        if fresh:
            ctx.set_option("sivm_sgreedy", 1)
        return ctx

    def _take_select(self, ctx):
        self.select = reference_order(ctx.get_select())        # (the device has ordered it already: W and H follow that order)
        self._v = [float(v) for v in ctx.get_volumes()]
        self._t = [time.time() - self._stime] * (self._num_bases - 1)

    def update_w(self):                                        # sivm_sgreedy.py:96-133
        self._stime = time.time()
        SIVM.update_w(self)

    def factorize(self, show_progress=False, compute_w=True, compute_h=True, compute_err=True, niter=1):
        """Factorize s.t. WH = data; always one iteration (sivm.py:203-228)."""
        self._stime = time.time()
        SIVM.factorize(self, show_progress=show_progress, compute_w=compute_w, compute_h=compute_h, compute_err=compute_err,
                       niter=niter)
