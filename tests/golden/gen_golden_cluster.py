#!/usr/bin/env python3
"""Generate the Kmeans / Cmeans golden vectors (tests/golden/kmeans_*.npz, cmeans_*.npz) by running the REAL reference
pymf/kmeans.py and pymf/cmeans.py, imported unmodified through the shim of gen_golden.py plus one line:
  * sys.modules["dist"] = pymf.dist     (kmeans.py:14 and cmeans.py import `dist` as an implicit relative import)
The reference is fed float64 arrays holding float32-representable values; seeded V is stored by seed (load_golden rebuilds
it), blob data by the seed of tests/cluster_oracle.py:blobs.

k-means decides membership by comparing distances.  dist.vq is wrapped while the reference runs to record the smallest gap
(d2 - d1) / ||v|| between the best and the second-best centre over the whole run; only `random.seed` values whose gap is at
least 1e-4 are kept, and the gap is stored with the case.  The margin is derived: a float32 dot product of m <= 500 terms is
off by at most m 2^-24 = 3e-5 of ||w|| ||v|| in the worst case (about 1e-6 typically)."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import load_reference  # noqa: E402
from gen_golden_cnmf import seeded  # noqa: E402
from cluster_oracle import blobs  # noqa: E402

MIN_GAP = 1e-4


def load_cluster():
    load_reference()
    import importlib
    dist = importlib.import_module("pymf.dist")
    sys.modules["dist"] = dist
    return importlib.import_module("pymf.kmeans"), importlib.import_module("pymf.cmeans"), dist


def run_kmeans(kmeans, dist, V, k, rseed, niter, W=None, **kw):
    orig = dist.vq
    gaps = []

    def vq(A, B, metric="l2"):
        d = dist.pdist(A, B, metric=metric)
        if d.shape[0] > 1:
            s = np.sort(d, axis=0)
            vn = np.sqrt((np.asarray(B) ** 2).sum(axis=0))
            gaps.append(float(((s[1] - s[0]) / vn).min()))
        return orig(A, B, metric=metric)

    dist.vq = vq
    try:
        random.seed(rseed)
        mdl = kmeans.Kmeans(V.astype(np.float64), num_bases=k)
        if W is not None:
            mdl.W = W.copy()
        mdl.factorize(niter=niter, **kw)
    finally:
        dist.vq = orig
    return mdl, (min(gaps) if gaps else np.inf)


def main():
    kmeans, cmeans, dist = load_cluster()
    cases = {}

    def add_kmeans(name, V, desc, k, niter, seeds, W=None, **kw):
        for rs in seeds:
            mdl, gap = run_kmeans(kmeans, dist, V, k, rs, niter, W=W, **kw)
            if gap >= MIN_GAP:
                break
            print("%-28s random.seed(%d): gap %.2e < %.0e, next seed" % (name, rs, gap, MIN_GAP))
        else:
            raise RuntimeError("%s: no seed with a distance gap >= %g" % (name, MIN_GAP))
        d = dict(desc)
        d.update(k=np.int64(k), niter=np.int64(niter), random_seed=np.int64(rs), min_gap=np.float64(gap),
                 W=np.asarray(mdl.W, dtype=np.float64), assigned=np.asarray(mdl.assigned, dtype=np.int64),
                 compute_w=np.bool_(kw.get("compute_w", True)), compute_err=np.bool_(kw.get("compute_err", True)))
        if kw.get("compute_err", True):
            d["ferr"] = np.asarray(mdl.ferr, dtype=np.float64)
        if W is not None:
            d["W_user"] = np.asarray(W, dtype=np.float64)
        cases[name] = d                      # (H is the one-hot image of `assigned`: not stored)

    def add_cmeans(name, V, desc, k, niter, nseed, W=None, **kw):
        np.random.seed(nseed)
        mdl = cmeans.Cmeans(V.astype(np.float64), num_bases=k)
        if W is not None:
            mdl.W = W.copy()
        mdl.factorize(niter=niter, **kw)
        d = dict(desc)
        d.update(k=np.int64(k), niter=np.int64(niter), np_seed=np.int64(nseed), W=np.asarray(mdl.W, dtype=np.float64),
                 H=np.asarray(mdl.H, dtype=np.float64), ferr=np.asarray(mdl.ferr, dtype=np.float64),
                 compute_w=np.bool_(kw.get("compute_w", True)))
        if W is not None:
            d["W_user"] = np.asarray(W, dtype=np.float64)
        cases[name] = d

    def blob_case(m, n, nb, seed):
        V, W0, _ = blobs(m, n, nb, seed)
        return V, W0, dict(blob_seed=np.int64(seed), blob_shape=np.array([m, n, nb], dtype=np.int64))

    # the docstring's data (kmeans.py:48-50): a seed without an exact tie
    Vd = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]], dtype=np.float32)
    add_kmeans("kmeans_doc_2x3_k2", Vd, dict(V=Vd), 2, 10, seeds=range(0, 12))
    V, d = seeded(37, 29, 1, 0.0)
    add_kmeans("kmeans_37x29_k5", V, d, 5, 20, seeds=range(0, 4))
    add_kmeans("kmeans_37x29_k5_noerr", V, d, 5, 5, seeds=range(0, 4), compute_err=False)   # five iterations really run
    V, d = seeded(300, 64, 101, 0.3)
    add_kmeans("kmeans_300x64_k6", V, d, 6, 20, seeds=range(0, 4))
    V, d = seeded(500, 200, 104, 0.3)                            # n not a multiple of 16
    add_kmeans("kmeans_500x200_k12", V, d, 12, 20, seeds=range(0, 2))

    V, W0, d = blob_case(37, 29, 5, 201)
    add_cmeans("cmeans_37x29_k5", V, d, 5, 10, 7)
    V, W0, d = blob_case(300, 64, 6, 202)
    add_cmeans("cmeans_300x64_k6", V, d, 6, 10, 8)
    add_cmeans("cmeans_300x64_k6_userw", V, d, 6, 10, 9, W=W0, compute_w=False)

    for name, d in cases.items():
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
        print("%-28s %s len(ferr) %s of %d" % (name, "gap %.2e seed %d" % (float(d["min_gap"]), int(d["random_seed"]))
                                               if "min_gap" in d else "np seed %d" % int(d["np_seed"]),
                                               len(d["ferr"]) if "ferr" in d else "-", int(d["niter"])))


if __name__ == "__main__":
    main()
