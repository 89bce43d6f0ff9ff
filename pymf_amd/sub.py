"""pymf_amd.SUB -- pymf.SUB (reference pymf/sub.py) on MI355X: factorise a column sample, then compute H for all columns.

SUB chooses `nsub` columns of the data by a sampling strategy, runs the factorisation class `mfmethod` on that sample to get
W, and computes H for ALL columns with W fixed (sub.py:163-223).  It is the reference's answer to data too large to factorise
directly, so the full data are the expensive thing: per factorize() they cross the host link AT MOST ONCE.  The first model of
a call that needs them -- the selection model of 'kmeans', 'sivm', 'laesa' and 'cur', the full model of 'rand' -- is filled from
the host; every other model of the call is filled from that one's context on the device (pmf_set_v_gather_f32: the sample by
a column gather, the full model by the whole-copy form; NMF.adopt_data_from).  The full model of one call holds the data for
the next: a second factorize() on unchanged data uploads nothing, one after an in-place edit of `data` (check_data, NMF's
digest) uploads once.

The reference's SUB cannot run in its own fork (sub.py:51 passes keywords NMF.__init__ does not take; sub.py:117,146,153,175,187
call an initialization() that no longer exists; sub.py:160 uses xrange; 'hull' calls the quickhull that does not terminate), so
SUB is defined by what sub.py states:

  'rand' (and any unknown name)   random.sample(range(n), nsub), sorted (sub.py:160 with range for xrange)
  'cur'      probabilities from the float64 squared column norms of the resident data (pmf_cur_sqnorms), np.cumsum on the host,
             nsub np.random.rand() draws, each mapped to the first index with cumsum >= r (sub.py:133-141); repeats are kept; a
             draw beyond the last cumulative value (rounding) maps to the last column -- the reference's IndexError
  'kmeans'   Kmeans(data, num_bases=nsub).factorize(), then vq(kmeans_mdl, kmeans_mdl.W) against the resident data; nsub <= 128
  'sivm' / 'laesa'   SIVM / LAESA(data, num_bases=nsub, dist_measure='cosine').factorize(compute_h=False, compute_err=False),
             then .select; nsub <= 64, at most 16384 rows; an entry -1 (init='origin') is the last column
  'hull'     NotImplementedError from update_w (see CHNMF); the constructor accepts the name

update_w sorts the indices (np.sort(np.int32(idx)), sub.py:166), runs mfmethod(data[:, idx], num_bases=num_bases).factorize()
with the class's defaults (show_progress / compute_w of sub.py:169-172 are stored on SUB and not forwarded), binds
self.mdl = mfmethod(data, num_bases=num_bases) and gives it W: a copy of the sample's W, or (mapW) for each of its columns the
nearest data column by vq(self.mdl, W) (sub.py:189-201).  update_h runs self.mdl.factorize(niter=niterH, compute_w=False).
No initialization() is called, so the only random draws are the strategy's and those of the two factorize() calls.

Refused before any device call: an mfmethod that is not a pymf_amd model class (TypeError, by the constructor), scipy.sparse
data (TypeError), streamed data (ValueError), a multi-rank world (NotImplementedError), a strategy's own limit on nsub
(ValueError; 'rand': random.sample's).
"""
import inspect
import logging
import random

import numpy as np

from . import _lib
from .distance import vq
from .kmeans import Kmeans
from .laesa import LAESA
from .nmf import NMF, _is_sparse
from .sivm import SIVM

__all__ = ["SUB"]

_SIVM_MAX_ROWS = 16384


class _ColumnNorms(NMF):
    """Holds `data` on a CUR context, the family that forms the float64 squared norms (k_cur_sqnorms) and has no limit on
    the shape.  The selection model of the 'cur' strategy."""
    _ALGO = _lib.ALGO_CUR

    def column_sqnorms(self):
        return self._context().cur_sqnorms()[1]


class SUB(NMF):
    """
    SUB(data, mfmethod, nsub=20, show_progress=True, mapW=False, base_sel=2, num_bases=3, niterH=1, compute_h=True,
    compute_w=True, sstrategy='rand')

    >>> data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    >>> sub_mdl = SUB(data, pymf_amd.NMF, nsub=2, num_bases=2)
    >>> sub_mdl.factorize()

    The factorisation of all columns is sub_mdl.mdl; W, H and ferr (one entry: its Frobenius norm) are bound from it.
    """
    def __init__(self, data, mfmethod, nsub=20, show_progress=True, mapW=False, base_sel=2,
                 num_bases=3, niterH=1, compute_h=True, compute_w=True, sstrategy='rand'):
        if not (isinstance(mfmethod, type) and issubclass(mfmethod, NMF)) or issubclass(mfmethod, SUB):
            raise TypeError("SUB: mfmethod must be a pymf_amd model class (NMF, NMFALS, Kmeans, SIVM ...), not %r" % (mfmethod,))
        NMF.__init__(self, data, num_bases=num_bases)          # sub.py:51
        self._show_progress = show_progress
        self._compute_h = compute_h
        self._compute_w = compute_w
        self._niterH = niterH
        self._nsub = nsub
        self._mfmethod = mfmethod
        self._mapW = mapW
        self._sstrategy = sstrategy
        self._base_sel = base_sel
        self._holder = None       # the model whose context holds the full data: what the other models are filled from
        self._holder_checked = False
        self._subfunc = {'cur': self.curselect, 'kmeans': self.kmeansselect, 'hull': self.hullselect,       # sub.py:61-78
                         'laesa': self.laesaselect, 'sivm': self.sivmselect}.get(sstrategy, self.randselect)

    def __getstate__(self):
        st = NMF.__getstate__(self)
        st["_holder"], st["_holder_checked"] = None, False
        return st

    def _check_supported(self):
        if _is_sparse(self.data):
            raise TypeError("SUB: scipy.sparse data is not supported (dense data only)")
        if self.stream_rows or self._stream_rows():
            raise ValueError("SUB: streamed data (stream_rows) is not supported: the column gather needs the data resident")
        if self._world().size > 1:
            raise NotImplementedError("SUB: one rank only (a multi-rank world is not supported)")
        if self._nsub < 1:
            raise ValueError("SUB: nsub must be at least 1")

    # ---- where a model's device V comes from -------------------------------------------------------------------------
    def _fill(self, mdl, columns=None):
        """mdl's device V: gathered from the model that holds the full data, or -- when none does yet -- uploaded from the
        host (mdl then is that model).  The holder of an earlier call is asked once per call whether `data` still is what it
        holds (check_data: an in-place edit sends it up again)."""
        if self._holder is not None and not self._holder_checked:
            self._holder.upload_data()
            self._holder_checked = True
        if self._holder is None:
            if columns is not None:
                raise RuntimeError("SUB: a column sample can only be filled from a model that holds the data")
            mdl.upload_data()
            self._holder, self._holder_checked = mdl, True
        else:
            mdl.adopt_data_from(self._holder, columns)

    # ---- the strategies: each returns an index array -----------------------------------------------------------------
    def hullselect(self):                                      # sub.py:80-113
        raise NotImplementedError("SUB: sstrategy 'hull' is not supported (the reference's quickhull does not terminate); "
                                  "CHNMF selects hull points of the pairwise projections on the device")

    def kmeansselect(self):                                    # sub.py:115-122
        if self._nsub > Kmeans._MAX_BASES:
            raise ValueError("SUB: sstrategy 'kmeans' takes nsub <= %d (Kmeans: num_bases > %d is not supported)"
                             % (Kmeans._MAX_BASES, Kmeans._MAX_BASES))
        kmeans_mdl = Kmeans(self.data, num_bases=self._nsub)
        self._fill(kmeans_mdl)
        kmeans_mdl.factorize()
        return vq(kmeans_mdl, kmeans_mdl.W)                    # the data columns closest to the centres

    def _column_sqnorms(self):
        """The float64 squared column norms of the resident data."""
        norms_mdl = _ColumnNorms(self.data, num_bases=1)
        self._fill(norms_mdl)
        return norms_mdl.column_sqnorms()

    def curselect(self):                                       # sub.py:124-141
        pcol = np.asarray(self._column_sqnorms(), dtype=np.float64)
        pcol = pcol / pcol.sum()
        prob_cols = np.cumsum(pcol.flatten())
        temp_ind = np.zeros(self._nsub, np.int32)
        for i in range(self._nsub):
            # the first index with cumsum >= r (sub.py:138-139); beyond the last cumulative value: the last column
            temp_ind[i] = min(int(np.searchsorted(prob_cols, np.random.rand(), side='left')), prob_cols.shape[0] - 1)
        return np.sort(temp_ind)

    def _volume_select(self, cls):
        name = cls.__name__
        if self._nsub > cls._MAX_BASES:
            raise ValueError("SUB: sstrategy '%s' takes nsub <= %d (%s: num_bases > %d is not supported)"
                             % (name.lower(), cls._MAX_BASES, name, cls._MAX_BASES))
        if self._data_dimension > _SIVM_MAX_ROWS:
            raise ValueError("SUB: sstrategy '%s' takes at most %d rows (%s: data_dimension > %d is not supported)"
                             % (name.lower(), _SIVM_MAX_ROWS, name, _SIVM_MAX_ROWS))
        mdl = cls(self.data, num_bases=self._nsub, dist_measure='cosine')
        self._fill(mdl)
        mdl.factorize(compute_h=False, compute_err=False)
        idx = np.asarray(mdl.select, dtype=np.int64)
        return np.where(idx < 0, idx + self._num_samples, idx)  # -1 (init='origin'): the last column, as a Python index reads it

    def sivmselect(self):                                      # sub.py:143-149
        return self._volume_select(SIVM)

    def laesaselect(self):                                     # sub.py:151-156
        return self._volume_select(LAESA)

    def randselect(self):                                      # sub.py:159-161
        idx = random.sample(range(self._num_samples), self._nsub)
        return np.sort(np.int32(idx))

    # ---- the reference's hooks -----------------------------------------------------------------------------------------
    def update_w(self):                                        # sub.py:163-201
        self._check_supported()
        if self._holder is not None and self._holder.data is not self.data:
            self._holder = None                                # (`data` was rebound: nothing resident belongs to it)
        self._holder_checked = False
        try:
            idx = self._subfunc()
            idx = np.sort(np.int32(idx))                       # sub.py:166
            self._idx = idx                                    # (kept: the columns of the sample, ascending, repeats included)

            mdl_small = self._mfmethod(self.data[:, idx], num_bases=self._num_bases)
            self.mdl = self._mfmethod(self.data, num_bases=self._num_bases)
            self._fill(self.mdl)                               # ('rand': the one upload; else a whole copy on the device)
            self._fill(mdl_small, idx)
            mdl_small.factorize()                              # determine W

            if self._mapW:                                     # sub.py:189-199
                w_small = np.asarray(mdl_small.W)
                mapped = vq(self.mdl, w_small)
                w = np.zeros(w_small.shape)
                for i, s in enumerate(mapped):
                    w[:, i] = self.data[:, s]
                self.mdl.W = w
            else:
                self.mdl.W = np.copy(mdl_small.W)              # sub.py:201
        except BaseException:
            self._holder = None                                # (whatever was half filled: the next call starts from the host)
            raise
        self._holder = self.mdl                                # the selection model may go: the full model holds the data

    def update_h(self):                                        # sub.py:203-204
        if 'niter' in inspect.signature(self.mdl.factorize).parameters:
            self.mdl.factorize(niter=self._niterH, compute_w=False)
        else:
            self.mdl.factorize(compute_w=False)

    def frobenius_norm(self):
        return self.mdl.frobenius_norm() if 'mdl' in self.__dict__ else -123456

    def factorize(self):
        """W from the factorisation of a column sample, then H for all columns with W fixed (sub.py:206-223)."""
        self.update_w()
        if self._compute_h:
            self.update_h()
            self.H = self.mdl.H
        self.W = self.mdl.W

        self.ferr = np.zeros(1)
        self.ferr[0] = self.mdl.frobenius_norm()
        self._logger.setLevel(logging.INFO if self._show_progress else logging.ERROR)
        self._logger.info(' Fro:' + str(self.ferr[0]))         # sub.py:223
