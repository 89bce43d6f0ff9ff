#!/usr/bin/env python3
"""SIVM at 64 x 1 048 576, k = 64 on one MI355X: update_w (num_bases + 2 launches of k_sivm_pass) and update_h (rounds of
non-negative QPs), ten timed values each behind a warm-up call, median and spread; the achieved bytes per second of
k_sivm_pass against its algorithmic traffic 4 m np + 48 np per pass (the project's best streaming kernel, the SNMF W write,
reaches 6.6 TB/s), and one NMFALS update_h at the same shape beside the H step."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
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


def main():
    rs = np.random.RandomState(0)
    verts = 4.0 * np.linspace(1.0, 3.0, K) * np.linalg.qr(rs.randn(M, M))[0][:, :K]
    V = np.empty((M, N), dtype=np.float32)
    for c0 in range(0, N, 1 << 16):
        h = 0.8 * rs.dirichlet(np.full(K, 0.5), size=1 << 16).T + 0.2 / K
        V[:, c0:c0 + (1 << 16)] = verts.dot(h) + 0.12 * rs.randn(M, 1 << 16) / 8.0
    V[:, rs.choice(N, K, replace=False)] = verts
    ctx = _lib.Context(_lib.ALGO_SIVM, M, N, K)
    ctx.set_v_dense(V)
    ctx.profile_enable(True)
    w = timed(ctx.update_w)
    st = ctx.kernel_stats()
    ctx.profile_enable(False)
    h = timed(ctx.update_h)
    als = _lib.Context(_lib.ALGO_NMFALS, M, N, K)
    als.set_v_dense(V)
    als.set_w(ctx.get_w())
    als.set_h(np.zeros((K, N), dtype=np.float32))
    a = timed(als.update_h)
    print(json.dumps({"shape": [M, N, K], "update_w_ms": w, "update_h_ms": h, "nmfals_update_h_ms": a,
                      "h_step_over_nmfals": h[0] / a[0], "k_sivm_pass": st,
                      "k_sivm_pass_TBps": st["bytes_per_launch"] / (st["mean_ms"] * 1e-3) / 1e12 if st["mean_ms"] else None}))


if __name__ == "__main__":
    main()
