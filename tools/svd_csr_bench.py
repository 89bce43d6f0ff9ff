#!/usr/bin/env python3
"""SVD on CSR data (k_csr_gram, the Jacobi solver, k_csr_proj_f64; pmf_svd_csr.h) on one MI355X.

(a) 1 048 576 x 1 024 at 0.1 % stored entries, k = 64: behind one warm-up call, five runs of the pmf_svd_decompose call (host wall
    clock around the call, which returns with the device idle: the Gram matrix, the Jacobi solve, the gather and the projection
    are in it; pmf_invalidate_v in front of each so that it decomposes anew), and of k_csr_proj_f64 alone (pmf_profile_enable's
    event pair around its launch), in TB/s on its algorithmic bytes (12 nnz, the pointers, 8 r per output element; B from L2).
    The Gram matrix and the Jacobi solve have no profile site of their own: they are the call minus the projection, together.
(b) The yardstick, 65 536 x 1 024 at 1 % stored entries, k = 64: the dense SVD on toarray() and the sparse path on the same matrix,
    in one process, alternating within each of five runs behind one warm-up run.
Writes profiles/svd_csr_bench.json (or the path given).  `--small` runs both parts at 1/64 of the rows (a plumbing check)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pymf_amd import _lib  # noqa: E402
from cur_csr_bench import poisson_csr, stats, timed_ms  # noqa: E402

RUNS, K = 5, 64


def free_bytes():
    import ctypes
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def decompose(ctx):
    ctx.invalidate_v()
    return ctx.svd_decompose()


def big_shape(V):
    m, n = V.shape
    before = free_bytes()
    ctx = _lib.Context(_lib.ALGO_PCA, m, n, min(m, n))
    try:
        ctx.set_option("svd_num_triples", K)
        upload_ms, _ = timed_ms(lambda: ctx.set_v_csr(V.indptr, V.indices, V.data))
        assert ctx.path_name == "svd_csr"
        rank = decompose(ctx)                                     # warm-up
        device_bytes = before - free_bytes()                      # the context with CSR data and one decomposition (the slabs of k_csr_gram included)
        call_ms, proj_ms = [], []
        for _ in range(RUNS):
            call_ms.append(timed_ms(lambda: decompose(ctx))[0])
            ctx.profile_enable(True)
            decompose(ctx)
            st = ctx.kernel_stats()
            each = ctx.kernel_launch_ms()
            ctx.profile_enable(False)
            assert st["name"] == "k_csr_proj_f64" and len(each) == 1, (st, len(each))
            proj_ms.append(float(each[0]))
        ferr_ms, ferr = timed_ms(ctx.frobenius)
        rp = -(-rank // 64) * 64
        lines = -(-max(m, n) // 64) * 64
        alg_bytes = 12.0 * V.nnz + 8.0 * lines + 8.0 * rp * lines
        return {"shape": [m, n, K], "rank": rank, "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "set_v_csr_ms": upload_ms,
                "device_bytes": device_bytes, "dense_image_bytes": 4 * m * n,
                "svd_decompose_call_ms": stats(call_ms), "k_csr_proj_f64_ms": stats(proj_ms), "k_csr_proj_f64_bytes": alg_bytes,
                "k_csr_proj_f64_TBps": alg_bytes / (float(np.median(proj_ms)) * 1e-3) / 1e12,
                "gram_and_jacobi_ms": "not measured separately (no profile site): the call minus the projection",
                "frobenius_call_ms": ferr_ms, "ferr_over_norm": ferr / float(np.sqrt(np.sum(V.data.astype(np.float64) ** 2)))}
    finally:
        ctx.close()


def yardstick(V):
    m, n = V.shape
    ctxs = {"dense": _lib.Context(_lib.ALGO_PCA, m, n, min(m, n)), "sparse": _lib.Context(_lib.ALGO_PCA, m, n, min(m, n))}
    try:
        ctxs["sparse"].set_option("svd_num_triples", K)
        ctxs["dense"].set_v_dense(V.toarray())
        ctxs["sparse"].set_v_csr(V.indptr, V.indices, V.data)
        paths = {label: ctx.path_name for label, ctx in ctxs.items()}
        ms = {label: [] for label in ctxs}
        rank = {}
        for run in range(RUNS + 1):                              # run 0: warm-up, not recorded
            for label, ctx in ctxs.items():
                a, rank[label] = timed_ms(lambda: decompose(ctx))
                if run:
                    ms[label].append(a)
        # (pmf_svd_get writes as many values as the decomposition kept: the dense one keeps every triple above the cut)
        Sd, Ss = (ctxs[label].svd_get(rank[label], want="S")[1][:K] for label in ("dense", "sparse"))
        res = {"shape": [m, n, K], "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "paths": paths,
               "rank": rank, "svd_decompose_call_ms": {label: stats(v) for label, v in ms.items()},
               "S_sparse_vs_dense_rel_max": float(np.max(np.abs(Ss - Sd) / Sd))}
        res["svd_decompose_call_ms"]["dense_over_sparse"] = (res["svd_decompose_call_ms"]["dense"]["median"]
                                                             / res["svd_decompose_call_ms"]["sparse"]["median"])
        return res
    finally:
        for ctx in ctxs.values():
            ctx.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--small"]
    small = "--small" in sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "svd_csr_bench.json")
    shift = 6 if small else 0
    res = {"runs": RUNS, "small": small,
           "large": big_shape(poisson_csr((1 << 20) >> shift, 1 << 10, 1e-3, 1)),
           "yardstick": yardstick(poisson_csr((1 << 16) >> shift, 1 << 10, 1e-2, 3))}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
