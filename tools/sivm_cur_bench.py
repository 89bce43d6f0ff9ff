#!/usr/bin/env python3
"""SIVM_CUR at 64 x 1 048 576, 64 rows and columns on one MI355X: the factorize() call, the two selections alone (rows: the
long-sample pass on the resident data; columns: k_sivm_pass), ten timed values each behind a warm-up call, median and spread;
the mean time of one long-sample round (k_sivm_rowdist<l2> + k_sivm_rowstep) and its achieved bytes per second against its
algorithmic traffic, and, measured in the same run on the same data, one k_sivm_pass<l2> launch: both rounds read the same
268 MB.  Writes profiles/sivm_cur_bench.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pymf_amd  # noqa: E402
from pymf_amd import _lib  # noqa: E402

M, N, K, REPS = 64, 1 << 20, 64, 10


def timed(fn):
    fn()                                   # warm-up
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def pass_stats(ctx, fn):
    ctx.profile_enable(True)
    fn()
    st = ctx.kernel_stats()
    ctx.profile_enable(False)
    st["TBps"] = st["bytes_per_launch"] / (st["mean_ms"] * 1e-3) / 1e12 if st.get("mean_ms") else None
    return st


def main():
    rs = np.random.RandomState(0)
    V = np.empty((M, N), dtype=np.float32)
    left = rs.randn(M, M) * np.linspace(3.0, 0.3, M)
    for c0 in range(0, N, 1 << 16):
        V[:, c0:c0 + (1 << 16)] = left.dot(rs.randn(M, 1 << 16)) / 8.0
    mdl = pymf_amd.SIVM_CUR(V, rrank=K)
    out = {"shape": [M, N, K], "factorize_ms": timed(mdl.factorize)}
    out["distinct_rows"], out["distinct_cols"] = len(set(mdl._rid)), len(set(mdl._cid))
    ctx = _lib.Context(_lib.ALGO_CUR, M, N, K)
    ctx.set_v_dense(V)
    out["select_rows_ms"] = timed(lambda: ctx.sivm_select(K, True, 0, 1))
    out["select_cols_ms"] = timed(lambda: ctx.sivm_select(K, False, 0, 1))
    assert ctx.sivm_select(K, True, 0, 1).tolist() == mdl._rid and ctx.sivm_select(K, False, 0, 1).tolist() == mdl._cid
    ctx.set_option("profile_sivm_rows", 1)
    rows = pass_stats(ctx, lambda: ctx.sivm_select(K, True, 0, 1))
    ctx.close()
    out["long_sample_round"] = rows
    sv = _lib.Context(_lib.ALGO_SIVM, M, N, K)
    sv.set_v_dense(V)
    out["k_sivm_pass"] = pass_stats(sv, sv.update_w)
    sv.close()
    if rows.get("mean_ms") and out["k_sivm_pass"].get("mean_ms"):
        out["long_sample_round_over_k_sivm_pass"] = rows["mean_ms"] / out["k_sivm_pass"]["mean_ms"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sivm_cur_bench.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
