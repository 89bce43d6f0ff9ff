#!/usr/bin/env python3
"""SIVM on CSC data (k_sivm_csc_pass, k_csc_wtv: pmf_sivm_csc.h) on one MI355X.

(a) 16 384 x 1 048 576 at 0.1 % stored entries (16 per column, one in each block of 1 024 rows), 64 bases, 'l2', 'fastmap':
    behind one warm-up call, five runs of pmf_update_w -- the wall-clock time of the call (it synchronises) -- and of a
    profiled pmf_update_w (an event pair around each of the 66 launches of k_sivm_csc_pass<l2>: median per pass), with the
    bandwidth on the pass's algorithmic bytes: 8 nnz (value and row id) + 24 n (indptr, score) + 48 n (three float64 state
    arrays read and written).  Then the H step (k_csc_wtv and the multiplier search over 1 048 576 columns): wall clock of two
    pmf_update_h calls, or the library's message if it gives up.
(b) The yardstick, 16 384 x 32 768 at the same density (the dense image is 2 GiB): dense k_sivm_pass<l2> on toarray() and
    k_sivm_csc_pass<l2> on the CSC arrays, in the same process, alternating within each of five runs behind one warm-up run:
    update_w wall clock and the profiled median per pass, median and range.
Writes profiles/sivm_csc_bench.json (or the path given).  `--small` runs both parts with 1/64 of the columns (a plumbing check)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

RUNS, K = 5, 64


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)),
            "range": float(max(values) - min(values))}


def strata_csc(m, n, per_col, seed):
    """CSC arrays of an m x n matrix with per_col entries in every column, one at a uniform row of each of per_col equal blocks
    of rows (ascending, distinct), values in [0.05, 1.05)."""
    rs = np.random.RandomState(seed)
    block = m // per_col
    rows = (np.arange(per_col, dtype=np.int64)[None, :] * block + rs.randint(0, block, size=(n, per_col))).astype(np.int32).reshape(-1)
    indptr = np.arange(n + 1, dtype=np.int64) * per_col
    vals = (rs.random_sample(n * per_col) + 0.05).astype(np.float32)
    return indptr, rows, vals


def pass_bytes(nnz, n):
    return 8.0 * nnz + 24.0 * n + 48.0 * n


def timed_update_w(ctx):
    t0 = time.perf_counter()
    ctx.update_w()
    return (time.perf_counter() - t0) * 1e3


def profiled_pass_ms(ctx, want):
    ctx.profile_enable(True)
    ctx.update_w()
    st = ctx.kernel_stats()
    each = ctx.kernel_launch_ms()
    ctx.profile_enable(False)
    assert st["name"].startswith(want) and len(each) == K + 2, (st, len(each))
    return float(np.median(each)), st["name"]


def big_shape(m, n, per_col):
    indptr, rows, vals = strata_csc(m, n, per_col, 1)
    nnz = int(indptr[-1])
    ctx = _lib.Context(_lib.ALGO_SIVM, m, n, K)
    try:
        ctx.set_v_csc(indptr, rows, vals)
        path = ctx.path_name
        ctx.update_w()                                           # warm-up
        call_ms, pass_ms = [], []
        for _ in range(RUNS):
            call_ms.append(timed_update_w(ctx))
            p, name = profiled_pass_ms(ctx, "k_sivm_csc_pass<l2>")
            pass_ms.append(p)
        res = {"shape": [m, n, K], "nnz": nnz, "density": nnz / float(m) / n, "path": path, "kernel": name,
               "update_w_ms": stats(call_ms), "pass_ms": stats(pass_ms)}
        res["pass_ms"]["algorithmic_bytes"] = pass_bytes(nnz, n)
        res["pass_ms"]["TBps"] = res["pass_ms"]["algorithmic_bytes"] / (res["pass_ms"]["median"] * 1e-3) / 1e12
        try:
            h_ms = []
            for _ in range(2):
                t0 = time.perf_counter()
                ctx.update_h()
                h_ms.append((time.perf_counter() - t0) * 1e3)
            res["update_h_ms"] = stats(h_ms)
        except _lib.PmfError as e:
            res["update_h_error"] = str(e)
        return res
    finally:
        ctx.close()


def yardstick(m, n, per_col):
    indptr, rows, vals = strata_csc(m, n, per_col, 3)
    dense = np.zeros((m, n), dtype=np.float32)
    dense[rows, np.repeat(np.arange(n), per_col)] = vals
    ctxs = {"dense": _lib.Context(_lib.ALGO_SIVM, m, n, K), "sparse": _lib.Context(_lib.ALGO_SIVM, m, n, K)}
    want = {"dense": "k_sivm_pass<l2>", "sparse": "k_sivm_csc_pass<l2>"}
    try:
        ctxs["dense"].set_v_dense(dense)
        ctxs["sparse"].set_v_csc(indptr, rows, vals)
        del dense
        paths = {label: ctx.path_name for label, ctx in ctxs.items()}
        call_ms = {label: [] for label in ctxs}
        pass_ms = {label: [] for label in ctxs}
        selects = {}
        for run in range(RUNS + 1):                              # run 0: warm-up, not recorded
            for label, ctx in ctxs.items():
                t = timed_update_w(ctx)
                p, _ = profiled_pass_ms(ctx, want[label])
                selects[label] = ctx.get_select().tolist()
                if run:
                    call_ms[label].append(t)
                    pass_ms[label].append(p)
        res = {"shape": [m, n, K], "nnz": int(indptr[-1]), "density": int(indptr[-1]) / float(m) / n, "paths": paths,
               "same_selection": selects["dense"] == selects["sparse"],
               "update_w_ms": {label: stats(v) for label, v in call_ms.items()},
               "pass_ms": {label: stats(v) for label, v in pass_ms.items()}}
        res["dense_over_sparse_pass"] = res["pass_ms"]["dense"]["median"] / res["pass_ms"]["sparse"]["median"]
        return res
    finally:
        for ctx in ctxs.values():
            ctx.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--small"]
    small = "--small" in sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "sivm_csc_bench.json")
    shift = 6 if small else 0
    res = {"runs": RUNS, "small": small,
           "large": big_shape(1 << 14, (1 << 20) >> shift, 16),
           "yardstick": yardstick(1 << 14, (1 << 15) >> shift, 16)}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
