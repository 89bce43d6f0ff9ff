#!/usr/bin/env python3
"""NMF on CSR data (k_nmf_sp_step, pmf_nmf_csr.h) on one MI355X.

(a) 1 048 576 x 16 384 at 0.1 % stored entries, k = 64 and k = 128: behind one warm-up call, five runs of an unprofiled
    pmf_factorize (ITERS iterations, both half steps; the loop's own HIP events give the time of an iteration) and of a
    profiled one (an event pair around every launch of the kernel: even launches are W steps, odd ones H steps).  Per half
    step: median and range of the time, the bandwidth on the kernel's algorithmic bytes -- 12 B per stored entry for the CSR
    arrays, X read and written, nnz KP 4 bytes of gathered rows of Y -- and the share of an iteration that is spent outside
    k_nmf_sp_step (the two slab sums, launch gaps).
(b) The yardstick, 65 536 x 4 096 at 1 % stored entries, k = 64: the dense NMF path on toarray() and the sparse path on the
    same matrix, in the same process, alternating within each of five runs behind one warm-up run; per-iteration time of
    pmf_factorize from the loop's events, median and range.
Writes profiles/nmf_csr_bench.json (or the path given).  `--small` runs both parts at 1/64 of the rows (a plumbing check)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

RUNS, ITERS = 5, 10


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)),
            "range": float(max(values) - min(values))}


def poisson_csr(m, n, density, seed):
    """CSR arrays of an m x n matrix whose rows hold Poisson(density n) entries at uniform columns (sorted within a row; a
    column drawn twice stays twice: duplicates add up), values in [0.05, 1.05)."""
    rs = np.random.RandomState(seed)
    counts = rs.poisson(density * n, size=m).astype(np.int64)
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    nnz = int(indptr[-1])
    key = np.repeat(np.arange(m, dtype=np.int64), counts) * n + rs.randint(0, n, size=nnz)
    key.sort()
    indices = (key % n).astype(np.int32)
    vals = (rs.random_sample(nnz) + 0.05).astype(np.float32)
    return indptr, indices, vals


def kp_of(k):
    return 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128


def half_step_bytes(nnz, rows, kp):
    return 12.0 * nnz + 8.0 * rows * kp + 4.0 * nnz * kp


def big_shape(m, n, density, k, csr):
    indptr, indices, vals = csr
    nnz = int(indptr[-1])
    ctx = _lib.Context(_lib.ALGO_NMF, m, n, k)
    try:
        ctx.set_v_csr(indptr, indices, vals)
        ctx.fill_w_uniform(1)
        ctx.fill_h_uniform(2)
        assert ctx.path_name.startswith("nmf_csr_gather")
        ctx.factorize(2, compute_err=False)                      # warm-up
        it_ms, w_ms, h_ms = [], [], []
        for _ in range(RUNS):
            ctx.factorize(ITERS, compute_err=False)
            it_ms.append(ctx.last_loop_ms() / ITERS)
            ctx.profile_enable(True)
            ctx.factorize(ITERS, compute_err=False)
            st = ctx.kernel_stats()
            each = ctx.kernel_launch_ms()
            ctx.profile_enable(False)
            assert st["name"].startswith("k_nmf_sp_step") and len(each) == 2 * ITERS, (st, len(each))
            w_ms.append(float(np.median(each[0::2])))
            h_ms.append(float(np.median(each[1::2])))
        kp = kp_of(k)
        res = {"shape": [m, n, k], "nnz": nnz, "density": nnz / float(m) / n, "kernel": st["name"],
               "iteration_ms": stats(it_ms), "w_step_ms": stats(w_ms), "h_step_ms": stats(h_ms)}
        for key, rows in (("w_step_ms", m), ("h_step_ms", n)):
            res[key]["algorithmic_bytes"] = half_step_bytes(nnz, rows, kp)
            res[key]["TBps"] = res[key]["algorithmic_bytes"] / (res[key]["median"] * 1e-3) / 1e12
        res["share_outside_kernel"] = 1.0 - (res["w_step_ms"]["median"] + res["h_step_ms"]["median"]) / res["iteration_ms"]["median"]
        return res
    finally:
        ctx.close()


def yardstick(m, n, density, k):
    indptr, indices, vals = poisson_csr(m, n, density, 3)
    import scipy.sparse as sp
    V = sp.csr_matrix((vals, indices, indptr), shape=(m, n))
    V.sum_duplicates()
    dense = V.toarray()
    ctxs = {"dense": _lib.Context(_lib.ALGO_NMF, m, n, k), "sparse": _lib.Context(_lib.ALGO_NMF, m, n, k)}
    try:
        ctxs["dense"].set_v_dense(dense)
        ctxs["sparse"].set_v_csr(V.indptr, V.indices, V.data)
        paths = {}
        for label, ctx in ctxs.items():
            ctx.fill_w_uniform(1)
            ctx.fill_h_uniform(2)
            paths[label] = ctx.path_name
        ms = {label: [] for label in ctxs}
        for run in range(RUNS + 1):                              # run 0: warm-up, not recorded
            for label, ctx in ctxs.items():
                ctx.factorize(ITERS, compute_err=False)
                if run:
                    ms[label].append(ctx.last_loop_ms() / ITERS)
        res = {"shape": [m, n, k], "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "paths": paths,
               "iteration_ms": {label: stats(v) for label, v in ms.items()}}
        res["dense_over_sparse"] = res["iteration_ms"]["dense"]["median"] / res["iteration_ms"]["sparse"]["median"]
        return res
    finally:
        for ctx in ctxs.values():
            ctx.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--small"]
    small = "--small" in sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "nmf_csr_bench.json")
    m, n, density = (1 << 20) >> (6 if small else 0), 1 << 14, 1e-3
    csr = poisson_csr(m, n, density, 1)
    res = {"runs": RUNS, "iterations_per_run": ITERS, "small": small,
           "large": [big_shape(m, n, density, k, csr) for k in (64, 128)],
           "yardstick": yardstick((1 << 16) >> (6 if small else 0), 1 << 12, 1e-2, 64)}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
