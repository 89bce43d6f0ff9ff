#!/usr/bin/env python3
"""CURSL at 64 x 1 048 576 with rrank = 64 on one MI355X: the leverage pass k_lev_f64<true> beside its yardstick, the Gram
matrix k_prod_f64<false,sym> on the same data (a PCA context: the same bytes, the same flops), and k_cur_sqnorms, the pass that
CUR / CMD sample from -- five rounds, the three alternating in one process, each timed by HIP events around the launch in
calls of their own (pmf_profile_enable; pmf_set_option "profile_cur" chooses the launch on the CUR context).  Then, by the
host clock around calls that end in a synchronise, a few values each behind a warm-up call: pmf_cur_leverage with the
eigenpairs cached, pmf_cur_leverage behind a new upload of the same data (Gram matrix and Jacobi included; the upload itself is
not in the window) and CURSL.factorize().  Writes profiles/cursl_bench.json (or the path given as the first argument)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pymf_amd  # noqa: E402
from pymf_amd import _lib  # noqa: E402

M, N, R, REPS = 64, 1 << 20, 64, 5


def timed(fn, before=None):
    out = []
    for it in range(REPS + 1):             # the first is the warm-up
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if it:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def one_launch(ctx, fn):
    """kernel_stats() of the context's profiled site over one call of fn."""
    ctx.profile_enable(True)
    fn()
    st = ctx.kernel_stats()
    ctx.profile_enable(False)
    return st


def rates(us, st):
    s = us * 1e-6
    return {"us": us, "TBps": st["bytes_per_launch"] / s / 1e12, "TFLOPs": st["flops_per_launch"] / s / 1e12}


def main():
    rs = np.random.RandomState(0)
    V = rs.random_sample((M, N)).astype(np.float32)
    ctx = _lib.Context(_lib.ALGO_CUR, M, N, R)
    ctx.set_v_dense(V)
    pca = _lib.Context(_lib.ALGO_PCA, M, N, M)
    pca.set_v_dense(V)
    lev = lambda: ctx.cur_leverage(R, R)    # noqa: E731

    def decompose():
        pca.invalidate_v()                 # (a decomposition of unchanged data is kept)
        pca.svd_decompose()
    row, col = lev()                       # warm-up of all three
    decompose()
    ctx.cur_sqnorms()
    runs = {"k_lev_f64": [], "k_gram_f64": [], "k_cur_sqnorms": []}
    stats = {}
    for _ in range(REPS):
        ctx.set_option("profile_cur", 1)
        stats["k_lev_f64"] = one_launch(ctx, lev)
        runs["k_lev_f64"].append(stats["k_lev_f64"]["mean_ms"] * 1e3)
        stats["k_gram_f64"] = one_launch(pca, decompose)
        runs["k_gram_f64"].append(stats["k_gram_f64"]["mean_ms"] * 1e3)
        ctx.set_option("profile_cur", 2)
        stats["k_cur_sqnorms"] = one_launch(ctx, ctx.cur_sqnorms)
        runs["k_cur_sqnorms"].append(stats["k_cur_sqnorms"]["mean_ms"] * 1e3)
    ctx.set_option("profile_cur", 0)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    call_cached = timed(lev)
    call_fresh = timed(lev, before=lambda: ctx.set_v_dense(V))
    mdl = pymf_amd.CURSL(V, rrank=R)

    def factorize():
        np.random.seed(1)
        mdl.factorize()
    fact = timed(factorize)

    def what(st):                          # the launch's name and its algorithmic figures; the times are in kernel_us_runs
        return {k: st[k] for k in ("name", "flops_per_launch", "bytes_per_launch", "executed_flops_per_launch")}

    def mmm(t):
        return {"median": t[0], "min": t[1], "max": t[2]}
    out = {"shape": [M, N], "rrank": R, "reps": REPS,
           "kernel_us_runs": runs, "kernel_us_median": med,
           "k_lev_f64": what(stats["k_lev_f64"]), "k_lev_f64_rates_at_median": rates(med["k_lev_f64"], stats["k_lev_f64"]),
           "yardstick_k_gram_f64": what(stats["k_gram_f64"]),
           "yardstick_k_gram_f64_rates_at_median": rates(med["k_gram_f64"], stats["k_gram_f64"]),
           "k_cur_sqnorms": what(stats["k_cur_sqnorms"]), "k_cur_sqnorms_rates_at_median": rates(med["k_cur_sqnorms"], stats["k_cur_sqnorms"]),
           "k_lev_f64_over_k_gram_f64_medians": med["k_lev_f64"] / med["k_gram_f64"],
           "pmf_cur_leverage_call_ms_eigenpairs_cached": mmm(call_cached), "pmf_cur_leverage_call_ms_new_data": mmm(call_fresh),
           "CURSL_factorize_ms": mmm(fact), "ferr": float(mdl.frobenius_norm()),
           "leverage_sums": [float(row.sum()), float(col.sum())]}
    print(json.dumps(out))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cursl_bench.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
