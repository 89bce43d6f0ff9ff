#!/usr/bin/env python3
"""GREEDY at 64 x 1 048 576, 64 bases on one MI355X: update_w (64 rounds of k_greedy_pass and k_greedy_step behind the Gram
matrix and its eigenpairs) and update_h (H = pinv(W) data), ten timed values each behind a warm-up call, median and spread;
the mean time of one k_greedy_pass launch (the rounds use 4 to 8 operand tiles) and its achieved bytes per second against its
algorithmic traffic, and, measured in the same run on the same data, one k_aa_price<4> and one k_sivm_pass<l2> launch: the two
other passes over column panels that read the same 268 MB.  Writes profiles/greedy_bench.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ctx = _lib.Context(_lib.ALGO_GREEDY, M, N, K)
    ctx.set_v_dense(V)
    w = timed(ctx.update_w)
    sel = ctx.get_select().tolist()
    gp = pass_stats(ctx, ctx.update_w)
    h = timed(ctx.update_h)
    out = {"shape": [M, N, K], "update_w_ms": w, "update_h_ms": h, "distinct_selected": len(set(sel)), "k_greedy_pass": gp}
    sv = _lib.Context(_lib.ALGO_SIVM, M, N, K)
    sv.set_v_dense(V)
    out["k_sivm_pass"] = pass_stats(sv, sv.update_w)
    sv.close()
    aa = _lib.Context(_lib.ALGO_AA, M, N, K)
    aa.set_v_dense(V)
    aa.set_h(rs.rand(K, N).astype(np.float32))
    try:
        out["k_aa_price"] = pass_stats(aa, aa.update_w)
    except _lib.PmfError as e:             # (the W step may give up on its round cap: the launches before that were timed)
        out["k_aa_price"] = dict(aa.kernel_stats(), note=str(e))
    aa.close()
    for other in ("k_sivm_pass", "k_aa_price"):
        if out[other].get("mean_ms") and gp.get("mean_ms"):
            out["greedy_pass_over_" + other] = gp["mean_ms"] / out[other]["mean_ms"]
    ctx.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "greedy_bench.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
