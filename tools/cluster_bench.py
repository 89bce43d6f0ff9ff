#!/usr/bin/env python3
"""Kmeans / Cmeans timings on the device: ms per iteration of the loop (pmf_factorize, HIP events) and the achieved GB/s
counted on ONE read of V per iteration, at the shapes of DESIGN.md 3.11; optionally the float64 NumPy oracle's time per
iteration (measured on at most --oracle-cols columns and scaled to n: its cost is linear in n).
Kernel-level numbers: run it under `rocprofv3 --kernel-trace --stats -- python tools/cluster_bench.py`.

    python tools/cluster_bench.py [--oracle] [--shapes 64x1048576x16,...] [--niter 10] [--algos kmeans,cmeans]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ("64x1048576x16,64x1048576x64,64x1048576x128,256x262144x16,256x262144x64,256x262144x128,"
          "1048576x256x64")


def one(algo, m, n, k, niter, with_oracle, oracle_cols):
    from pymf_amd import _lib
    ctx = _lib.Context(_lib.ALGO_KMEANS if algo == "kmeans" else _lib.ALGO_CMEANS, m, n, k)
    ctx.fill_v_uniform(7)
    ctx.fill_w_uniform(8)
    ctx.fill_h_uniform(9)
    ctx.update_h()                              # Kmeans.init_h; warm-up
    out = dict(algo=algo, shape="%dx%d" % (m, n), k=k, path=ctx.path_name())
    for err in (False, True):
        ctx.factorize(1, True, True, err, conv_eps=-1.0)
        _, done, _ = ctx.factorize(niter, True, True, err, conv_eps=-1.0)
        ms = ctx.last_loop_ms() / max(done, 1)
        key = "with_err" if err else "no_err"
        out["ms_per_iter_" + key] = ms
        out["v_gbps_" + key] = 4.0 * m * n / (ms * 1e-3) / 1e9
    ctx.close()
    if with_oracle:
        import cluster_oracle as co
        nc = min(n, oracle_cols)
        rs = np.random.RandomState(7)
        Vd, W = rs.random_sample((m, nc)), rs.random_sample((m, k))
        t0 = time.perf_counter()
        if algo == "kmeans":
            co.kmeans(Vd, k, W=W, niter=1)
        else:
            co.cmeans(Vd, W, rs.random_sample((k, nc)), niter=1)
        out["oracle_ms_per_iter"] = (time.perf_counter() - t0) * 1e3 * n / nc
        out["oracle_cols"] = nc
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--algos", default="kmeans,cmeans")
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--oracle-cols", type=int, default=16384)
    a = ap.parse_args()
    for s in a.shapes.split(","):
        m, n, k = (int(x) for x in s.split("x"))
        for algo in a.algos.split(","):
            niter = 2 if m > 16 * n else a.niter        # the m >> n regime runs on a handful of workgroups
            print(json.dumps(one(algo, m, n, k, niter, a.oracle, a.oracle_cols)), flush=True)


if __name__ == "__main__":
    main()
