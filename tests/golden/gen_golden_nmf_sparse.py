#!/usr/bin/env python3
"""Generate the golden vectors of NMF on scipy.sparse data (tests/golden/nmfsp_*.npz) by running the REAL reference
pymf/nmf.py, imported unmodified through load_reference of gen_golden.py, on V.toarray(): the reference cannot run on the
sparse matrix itself (UFuncTypeError at nmf.py:131), and dense NMF on toarray() is the semantics pymf_amd.NMF states for
`accept_sparse = True`.

The reference is fed float64 arrays holding float32-representable values (V, W0, H0), so the device sees the same numbers.
Stored: V as CSR triplets (indptr, indices, data), the seed of the start (W0, H0 are drawn again by start() below, which
the test imports), W, H and niter.  W and H of a case that would pass 900 KB together go into two files (<name>.npz and
<name>_w.npz): no committed file above 1 MiB."""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# name: (m, n, k, density, niter, seed)
CASES = {
    "nmfsp_300x200_k6": (300, 200, 6, 0.05, 20, 101),
    "nmfsp_1000x520_k100": (1000, 520, 100, 0.02, 10, 102),     # the shape at which the SNMF CSR path expands to dense
}


def matrix(m, n, density, seed):
    """CSR, canonical, float64 values that float32 holds exactly, in [0.05, 1.05)."""
    rs = np.random.RandomState(seed)
    V = sp.random(m, n, density=density, format="csr", random_state=rs,
                  data_rvs=lambda size: (rs.random_sample(size) + 0.05).astype(np.float32).astype(np.float64))
    V.sum_duplicates()
    return V


def start(m, n, k, seed):
    """(W0, H0): float64 arrays of float32-representable values."""
    rs = np.random.RandomState(seed + 1000)
    W0 = rs.random_sample((m, k)).astype(np.float32).astype(np.float64)
    H0 = rs.random_sample((k, n)).astype(np.float32).astype(np.float64)
    return W0, H0


def main():
    from gen_golden import load_reference
    NMF = load_reference()["nmf"].NMF
    for name, (m, n, k, density, niter, seed) in CASES.items():
        V = matrix(m, n, density, seed)
        W0, H0 = start(m, n, k, seed)
        mdl = NMF(V.toarray(), num_bases=k)
        mdl.W, mdl.H = W0.copy(), H0.copy()
        mdl.factorize(niter=niter, compute_err=False)
        d = dict(indptr=V.indptr.astype(np.int64), indices=V.indices.astype(np.int32), data=V.data.astype(np.float32),
                 shape=np.array([m, n], dtype=np.int64), k=np.int64(k), niter=np.int64(niter), seed=np.int64(seed),
                 H=np.asarray(mdl.H, dtype=np.float64))
        W = np.asarray(mdl.W, dtype=np.float64)
        if W.nbytes + d["H"].nbytes > 900 * 1000:
            np.savez_compressed(os.path.join(HERE, name + "_w.npz"), W=W)
        else:
            d["W"] = W
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
        print("%-24s nnz %d (%.3g %%)  |W| %.6g  |H| %.6g" % (name, V.nnz, 100.0 * V.nnz / (m * n), np.linalg.norm(W),
                                                            np.linalg.norm(mdl.H)))


if __name__ == "__main__":
    main()
