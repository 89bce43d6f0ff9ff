#!/usr/bin/env python3
"""GREEDY on CSR data (k_csr_gram, the Jacobi solver, k_greedy_csr_pass + k_greedy_step_csr; pmf_greedy_csr.h) on one MI355X.

(a) 1 024 x 1 048 576 at 0.1 % stored entries, 64 bases: behind one warm-up call, five runs of the pmf_update_w call (host wall
    clock around the call, which returns with the device idle: the Gram matrix, the Jacobi solve, the 64 rounds and the gather of W
    are in it; pmf_invalidate_v in front of each so that the eigenpairs are formed anew), and the mean over the 64 rounds of
    k_greedy_csr_pass alone (pmf_profile_enable's event pairs around its launches).
(b) The yardstick, 1 024 x 32 768 at 1 % stored entries, 64 bases: the dense path on toarray() and the sparse path on the same
    matrix, in one process, alternating within each of five runs behind one warm-up run.
Writes profiles/greedy_csr_bench.json (or the path given).  `--small` runs both parts at 1/64 of the columns (a plumbing check)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pymf_amd import _lib  # noqa: E402
from cur_csr_bench import poisson_csr, stats, timed_ms  # noqa: E402
from svd_csr_bench import free_bytes  # noqa: E402

RUNS, K = 5, 64


def update_w(ctx):
    ctx.invalidate_v()
    ctx.update_w()
    return ctx.get_select()


def big_shape(V):
    m, n = V.shape
    before = free_bytes()
    ctx = _lib.Context(_lib.ALGO_GREEDY, m, n, K)
    try:
        upload_ms, _ = timed_ms(lambda: ctx.set_v_csr(V.indptr, V.indices, V.data))
        assert ctx.path_name == "greedy_csr"
        first = update_w(ctx)                                     # warm-up
        device_bytes = before - free_bytes()
        call_ms, pass_ms = [], []
        for _ in range(RUNS):
            a, sel = timed_ms(lambda: update_w(ctx))
            assert np.array_equal(sel, first)
            call_ms.append(a)
            ctx.profile_enable(True)
            update_w(ctx)
            st = ctx.kernel_stats()
            each = ctx.kernel_launch_ms()
            ctx.profile_enable(False)
            assert st["name"].startswith("k_greedy_csr_pass") and len(each) == K, (st, len(each))
            pass_ms.append(float(np.mean(each)))
        h_ms, _ = timed_ms(ctx.update_h)
        ferr_ms, ferr = timed_ms(ctx.frobenius)
        return {"shape": [m, n, K], "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "set_v_csr_ms": upload_ms,
                "device_bytes": device_bytes, "dense_image_bytes": 4 * m * n,
                "update_w_call_ms": stats(call_ms), "k_greedy_csr_pass_mean_ms_per_round": stats(pass_ms),
                "update_h_call_ms": h_ms, "frobenius_call_ms": ferr_ms,
                "ferr_over_norm": ferr / float(np.sqrt(np.sum(V.data.astype(np.float64) ** 2)))}
    finally:
        ctx.close()


def yardstick(V):
    m, n = V.shape
    ctxs = {"dense": _lib.Context(_lib.ALGO_GREEDY, m, n, K), "sparse": _lib.Context(_lib.ALGO_GREEDY, m, n, K)}
    try:
        ctxs["dense"].set_v_dense(V.toarray())
        ctxs["sparse"].set_v_csr(V.indptr, V.indices, V.data)
        paths = {label: ctx.path_name for label, ctx in ctxs.items()}
        ms = {label: [] for label in ctxs}
        sel = {}
        for run in range(RUNS + 1):                              # run 0: warm-up, not recorded
            for label, ctx in ctxs.items():
                a, sel[label] = timed_ms(lambda: update_w(ctx))
                if run:
                    ms[label].append(a)
        res = {"shape": [m, n, K], "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "paths": paths,
               "update_w_call_ms": {label: stats(v) for label, v in ms.items()},
               "leading_equal_selections": int(np.argmin(np.append(sel["dense"] == sel["sparse"], False)))}
        res["update_w_call_ms"]["dense_over_sparse"] = res["update_w_call_ms"]["dense"]["median"] / res["update_w_call_ms"]["sparse"]["median"]
        return res
    finally:
        for ctx in ctxs.values():
            ctx.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--small"]
    small = "--small" in sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "greedy_csr_bench.json")
    shift = 6 if small else 0
    res = {"runs": RUNS, "small": small,
           "large": big_shape(poisson_csr(1 << 10, (1 << 20) >> shift, 1e-3, 1)),
           "yardstick": yardstick(poisson_csr(1 << 10, (1 << 15) >> shift, 1e-2, 3))}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
