#!/usr/bin/env python3
"""AA at 64 x 1 048 576, k = 64 on one MI355X (the SIVM bench shape and data): update_w -- rounds of one k_aa_price pass over
V and one k_aa_master step per base -- and update_h, a few timed values each behind a warm-up call, median and spread; the
time of one k_aa_price pass (HIP events around every launch, in two update_w calls of their own, not the timed ones) and its achieved bytes per second against its algorithmic
traffic 4 m np, beside the yardstick k_sivm_pass<l2> at this shape (64 us, 4.96 TB/s: profiles/sivm_bench.json), which also
reads V once; the rounds one update_w takes.  H0 is the reference's init_h.  Writes profiles/aa_bench.json (or the path given as the first argument)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

M, N, K, REPS = 64, 1 << 20, 64, 5
SIVM_PASS_US, SIVM_PASS_TBPS = 64.0, 4.96


def timed(fn):
    fn()                                   # warm-up
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    rs = np.random.RandomState(0)
    verts = 4.0 * np.linspace(1.0, 3.0, K) * np.linalg.qr(rs.randn(M, M))[0][:, :K]
    V = np.empty((M, N), dtype=np.float32)
    for c0 in range(0, N, 1 << 16):
        h = 0.8 * rs.dirichlet(np.full(K, 0.5), size=1 << 16).T + 0.2 / K
        V[:, c0:c0 + (1 << 16)] = verts.dot(h) + 0.12 * rs.randn(M, 1 << 16) / 8.0
    V[:, rs.choice(N, K, replace=False)] = verts
    H0 = rs.random_sample((K, N)).astype(np.float32)
    H0 /= H0.sum(axis=0)
    ctx = _lib.Context(_lib.ALGO_AA, M, N, K)
    ctx.set_v_dense(V)
    ctx.set_h(H0)
    w = timed(ctx.update_w)                # (no events in the timed calls)
    rounds = ctx.aa_rounds()
    ctx.profile_enable(True)               # k_aa_price in calls of its own, HIP events around every launch
    ctx.update_w()
    ctx.update_w()
    st = ctx.kernel_stats()
    ctx.profile_enable(False)
    hstep = timed(ctx.update_h)
    ferr = ctx.frobenius()
    tbps = st["bytes_per_launch"] / (st["mean_ms"] * 1e-3) / 1e12 if st["mean_ms"] else None
    out = {"shape": [M, N, K], "reps": REPS, "update_w_ms": w, "update_h_ms": hstep, "rounds_per_update_w": rounds,
           "k_aa_price": st, "k_aa_price_us": st["mean_ms"] * 1e3, "k_aa_price_TBps": tbps,
           "k_aa_price_TFLOPs": st["flops_per_launch"] / (st["mean_ms"] * 1e-3) / 1e12 if st["mean_ms"] else None,
           "yardstick_k_sivm_pass_l2": {"us": SIVM_PASS_US, "TBps": SIVM_PASS_TBPS},
           "k_aa_price_over_k_sivm_pass": st["mean_ms"] * 1e3 / SIVM_PASS_US if st["mean_ms"] else None,
           "ferr_after_one_iteration": ferr}
    print(json.dumps(out))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "aa_bench.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
