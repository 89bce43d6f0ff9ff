#!/usr/bin/env python3
"""Generate the CNMF golden vectors (tests/golden/cnmf_*.npz) by running the REAL reference pymf/cnmf.py (with the k-means of
pymf/kmeans.py it initialises from), imported unmodified through the shim of gen_golden.py plus one line:
  * sys.modules["dist"] = pymf.dist     (kmeans.py:14 imports `dist` as an implicit relative import, Python 2 style)
The reference is fed float64 arrays holding float32-representable values (V is stored by seed: load_golden rebuilds it).

k-means decides cluster membership by comparing distances; the device compares them through C = V^T V, whose entries carry
about 1e-7 relative error.  dist.vq is wrapped while the reference runs to record the smallest relative gap (d2 - d1) / d2
between the best and the second-best centre over the whole k-means run; only random seeds whose gap is at least 1e-5 are
kept (about 30x the distance error), and the gap is stored with the case.
"""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import load_reference  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MIN_GAP = 1e-5


def load_cnmf():
    mods = load_reference()
    import importlib
    dist = importlib.import_module("pymf.dist")
    sys.modules["dist"] = dist
    cnmf = importlib.import_module("pymf.cnmf")
    return cnmf, dist


def seeded(m, n, seed, shift):
    V = (np.random.RandomState(seed).random_sample((m, n)) - shift).astype(np.float32)
    return V, dict(V_seed=np.int64(seed), V_shape=np.array([m, n], dtype=np.int64), V_shift=np.float64(shift))


def run(cnmf, dist, V, k, rseed, niter, W=None, compute_w=True, compute_h=True):
    """CNMF(V, k) with random.seed(rseed) -> (model, smallest relative gap seen by dist.vq)."""
    orig = dist.vq
    gaps = []

    def vq(A, B, metric="l2"):
        d = dist.pdist(A, B, metric=metric)
        s = np.sort(d, axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(s[1] > 0, (s[1] - s[0]) / s[1], 1.0)
        gaps.append(float(g.min()))
        return orig(A, B, metric=metric)

    dist.vq = vq
    try:
        random.seed(rseed)
        mdl = cnmf.CNMF(V.astype(np.float64), num_bases=k)
        if W is not None:
            mdl.W = W.copy()
        mdl.factorize(niter=niter, compute_w=compute_w, compute_h=compute_h)
    finally:
        dist.vq = orig
    return mdl, min(gaps)


def main():
    cnmf, dist = load_cnmf()
    cases = {}

    def add(name, V, desc, k, niter, seeds=range(0, 12), W=None, compute_w=True, compute_h=True, store=("W", "H", "G")):
        for rs in seeds:
            mdl, gap = run(cnmf, dist, V, k, rs, niter, W=W, compute_w=compute_w, compute_h=compute_h)
            if gap >= MIN_GAP:
                break
            print("%-28s random.seed(%d): gap %.2e < %.0e, next seed" % (name, rs, gap, MIN_GAP))
        else:
            raise RuntimeError("%s: no seed with a distance gap >= %g" % (name, MIN_GAP))
        d = dict(desc)
        d.update(k=np.int64(k), niter=np.int64(niter), random_seed=np.int64(rs), min_gap=np.float64(gap),
                 ferr=np.asarray(mdl.ferr, dtype=np.float64), compute_w=np.bool_(compute_w), compute_h=np.bool_(compute_h))
        for a in store:
            d[a] = np.asarray(getattr(mdl, a), dtype=np.float64)
        if W is not None:
            d["W_user"] = np.asarray(W, dtype=np.float64)
        cases[name] = d

    # the docstring's data (cnmf.py:51-53); random.seed(0) and (5) give exact ties there
    Vd = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]], dtype=np.float32)
    add("cnmf_doc_2x3_k2", Vd, dict(V=Vd), 2, 10, seeds=[1, 2, 3, 4, 6])
    V, d = seeded(300, 64, 101, 0.3)
    add("cnmf_300x64_k6_init", V, d, 6, 0)                      # k-means and init_h only
    add("cnmf_300x64_k6", V, d, 6, 30)
    rng = np.random.RandomState(102)
    Wu = rng.random_sample((300, 6))
    add("cnmf_300x64_k6_userw", V, d, 6, 10, W=Wu, compute_w=False)
    add("cnmf_300x64_k6_noh", V, d, 6, 10, compute_h=False)
    V, d = seeded(1000, 256, 103, 0.5)                           # zero-mean: neg(C) is not empty
    add("cnmf_1000x256_k16_mixed", V, d, 16, 50)
    V, d = seeded(500, 200, 104, 0.3)                            # n not a multiple of 16
    add("cnmf_500x200_k12", V, d, 12, 30)
    V, d = seeded(600, 512, 105, 0.3)
    add("cnmf_600x512_k128", V, d, 128, 5, store=("H", "G"))    # (W = V G: left out to keep the file small)
    V, d = seeded(20, 12, 107, 0.0)
    add("cnmf_20x12_k2_earlyexit", V, d, 2, 2000)               # stops at iteration 780 (nmf.py:134-139)

    for name, d in cases.items():
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
        print("%-28s seed %d gap %.2e len(ferr) %d of %d  ferr[-1] %s" % (
            name, int(d["random_seed"]), float(d["min_gap"]), len(d["ferr"]), int(d["niter"]),
            "%.9g" % d["ferr"][-1] if len(d["ferr"]) else "-"))


if __name__ == "__main__":
    main()
