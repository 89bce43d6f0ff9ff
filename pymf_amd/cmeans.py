"""pymf_amd.Cmeans -- drop-in for pymf.Cmeans (reference pymf/cmeans.py) on MI355X.

Fuzzy c-means as a factorization: W holds the centres, H the memberships.  update_h (cmeans.py:71-81), with
d = pdist(W, data) + 1e-8 and the fuzzifier m = 1.75: H[i] = 1 / sum_k (d[i] / d[k]) ** (2 / (m - 1)); update_w
(cmeans.py:83-86): W[:, i] = sum_c H[i, c] data[:, c] / (sum_c H[i, c] + 1e-8).  On the device one iteration is one pass over
the data, spread over column panels.  init_w, init_h (the np.random.random stream), factorize()'s loop, error,
convergence rule and the truncation of `ferr` are NMF's (nmf.py:116-120,171-202).

Supported: dense data of any shape, resident, one rank, num_bases <= 128.  scipy.sparse data raises TypeError, streamed data
(stream_rows) ValueError, a multi-rank world NotImplementedError, more than 128 bases ValueError.

scipy.sparse data: opt-in with `mdl.accept_sparse = True`, as for Kmeans (pymf_amd.kmeans): the data stay sparse
on the device, W and H come back dense, ferr is the float64 trace identity.
"""
from . import _lib
from .kmeans import _Clustering

__all__ = ["Cmeans"]


class Cmeans(_Clustering):
    _SHIPPED = True
    _ALGO = _lib.ALGO_CMEANS
