#!/usr/bin/env python3
"""CUR at 64 x 1 048 576 with 64 sampled rows and columns on one MI355X: the two calls of a factorize() -- pmf_cur_sqnorms
(one read of V by k_cur_sqnorms, its fixed-order reduce, m + n doubles to the host) and pmf_cur_compute (gather, the cross product k_prod_f64<false,full>,
the small products, two Gram matrices and Jacobi solves, W = C U and H = R) --, a few timed values each behind a warm-up call,
median and spread; the time of the cross product (HIP events around every launch, in calls of their own, not the timed ones) with its
achieved bytes and flops per second, beside its yardstick, the same kernel as Gram matrix (k_prod_f64<false,sym>) on the same data in the same process (a PCA
context: it moves the same bytes and flops).  The JSON keys keep the kernels' earlier names, k_cross_f64 and k_gram_f64, so
that old and new result files compare.  The time of k_cur_sqnorms alone is not taken here (one profiled site per
context): its call is to be read against k_sivm_pass<l2> at this shape (64 us, profiles/sivm_bench.json), which also reads V
once.  Writes profiles/cur_bench.json (or the path given as the first argument)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

M, N, R, REPS = 64, 1 << 20, 64, 5
SIVM_PASS_US = 64.0


def timed(fn):
    fn()                                   # warm-up
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def events(ctx, fn, calls=4):
    """kernel_stats() of the context's profiled site over `calls` calls of fn (after one warm-up call)."""
    fn()
    ctx.profile_enable(True)
    for _ in range(calls):
        fn()
    st = ctx.kernel_stats()
    ctx.profile_enable(False)
    return st


def rates(st):
    s = st["mean_ms"] * 1e-3
    return {"us": st["mean_ms"] * 1e3, "TBps": st["bytes_per_launch"] / s / 1e12 if s else None,
            "TFLOPs": st["flops_per_launch"] / s / 1e12 if s else None}


def main():
    rs = np.random.RandomState(0)
    V = rs.random_sample((M, N)).astype(np.float32)
    rid = np.sort(rs.choice(M, R, replace=False)).astype(np.int32)
    cid = np.sort(rs.choice(N, R, replace=False)).astype(np.int32)
    ones = np.ones(R, dtype=np.int32)
    ctx = _lib.Context(_lib.ALGO_CUR, M, N, R)
    ctx.set_v_dense(V)
    compute = lambda: ctx.cur_compute(rid, ones, cid, ones)    # noqa: E731
    norms_ms = timed(ctx.cur_sqnorms)
    compute_ms = timed(compute)
    cross = events(ctx, compute)
    ferr = ctx.frobenius()
    pca = _lib.Context(_lib.ALGO_PCA, M, N, M)
    pca.set_v_dense(V)

    def decompose():
        pca.invalidate_v()                 # (a decomposition of unchanged data is kept)
        pca.svd_decompose()
    gram = events(pca, decompose)
    out = {"shape": [M, N], "sampled_rows": R, "sampled_columns": R, "reps": REPS,
           "pmf_cur_sqnorms_call_ms": norms_ms, "pmf_cur_compute_call_ms": compute_ms,
           "k_cross_f64": cross, "k_cross_f64_rates": rates(cross),
           "yardstick_k_gram_f64": gram, "yardstick_k_gram_f64_rates": rates(gram),
           "k_cross_f64_over_k_gram_f64": cross["mean_ms"] / gram["mean_ms"] if gram["mean_ms"] else None,
           "yardstick_k_sivm_pass_l2_us": SIVM_PASS_US, "ferr": ferr}
    print(json.dumps(out))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cur_bench.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
