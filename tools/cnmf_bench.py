#!/usr/bin/env python3
"""CNMF timings on the device: the initialisation (C = V^T V plus the k-means, pmf_cnmf_init) and the loop per iteration
(pmf_factorize, HIP events), at the shapes of DESIGN.md 3.7; optionally the float64 NumPy oracle on the same shapes.
Kernel-level numbers: run it under `rocprofv3 --kernel-trace --stats -- python tools/cnmf_bench.py`.

    python tools/cnmf_bench.py [--oracle] [--shapes 1048576x256x64,4096x1024x128] [--niter 50]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def one(m, n, k, niter, with_oracle):
    from pymf_amd import _lib
    rs = np.random.RandomState(7)
    V = rs.random_sample((m, n)).astype(np.float32)
    random.seed(7)
    sel = np.sort(random.sample(range(n), k))
    ctx = _lib.Context(_lib.ALGO_CNMF, m, n, k)
    ctx.set_v_dense(V)
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.cnmf_init(sel, 10)                     # C + k-means + H, G (one call, blocking)
    t_init = (time.perf_counter() - t0) * 1e3
    ctx.factorize(2, True, True, True)         # warm-up (the first call also materialises W once)
    ferr, done, _ = ctx.factorize(niter, True, True, True, conv_eps=0.0)
    loop_ms = ctx.last_loop_ms()
    ferr1, _, _ = ctx.factorize(1, True, True, True, conv_eps=0.0)
    one_ms = ctx.last_loop_ms()                # one iteration + the W = V G write
    out = dict(shape="%dx%d" % (m, n), k=k, init_ms=t_init, loop_ms=loop_ms, iters=done,
               per_iter_ms=(loop_ms - one_ms) / max(done - 1, 1), w_write_plus_one_iter_ms=one_ms, ferr_last=float(ferr[done - 1]))
    ctx.close()
    if with_oracle:
        import cnmf_oracle
        Vd = V.astype(np.float64)
        t0 = time.perf_counter()
        H0, G0, _ = cnmf_oracle.cnmf_init(Vd, k, sel, vq_fn=cnmf_oracle.vq_gram if m * n > 1 << 24 else cnmf_oracle.vq)
        out["oracle_init_ms"] = (time.perf_counter() - t0) * 1e3
        it = 3
        t0 = time.perf_counter()
        cnmf_oracle.cnmf_factorize(Vd, H0, G0, niter=it)
        out["oracle_per_iter_ms"] = (time.perf_counter() - t0) * 1e3 / it
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1048576x256x64,4096x1024x128")
    ap.add_argument("--niter", type=int, default=50)
    ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    for s in a.shapes.split(","):
        m, n, k = (int(x) for x in s.split("x"))
        print(json.dumps(one(m, n, k, a.niter, a.oracle)), flush=True)


if __name__ == "__main__":
    main()
