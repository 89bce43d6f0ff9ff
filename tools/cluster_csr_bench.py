#!/usr/bin/env python3
"""Kmeans / Cmeans on CSR data (k_cluster_csr_assign, k_cluster_csr_num; pmf_cluster_csr.h) on one MI355X.

(a) `large`: 16 384 x 1 048 576 at 0.1 % stored entries, 64 bases, Kmeans and Cmeans: behind one warm-up iteration, five runs of
    one iteration (pmf_factorize with one iteration and no error: the W step, then the H step; host wall clock around the call,
    which returns with the device idle), and both kernels separately from the profile site (pmf_profile_enable's event pair
    around the launch of a pmf_update_h, then of a pmf_update_w).
(b) `yardstick`: 16 384 x 32 768 at the same density, 64 bases: the dense k_cluster_pass on toarray() against the sparse pair on
    the same matrix, in one process, alternating within each of five runs behind one warm-up run; the iteration's wall clock and
    the kernels' own times.
Each part runs as a call of its own (`python tools/cluster_csr_bench.py large|yardstick [out.json]`), so that a caller can give
each its own time limit; the parts are merged into profiles/cluster_csr_bench.json (or the path given).  `--small` runs a part at
1/64 of the columns (a plumbing check)."""
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
ALGOS = {"kmeans": _lib.ALGO_KMEANS, "cmeans": _lib.ALGO_CMEANS}


def start(ctx, V, seed):
    """W0 = K columns of the data (as Kmeans.init_w draws them), one H step: every later call finds W, H and the sums."""
    m, n = V.shape
    sel = np.sort(np.random.RandomState(seed).choice(n, K, replace=False))
    ctx.set_w(np.ascontiguousarray(V.tocsc()[:, sel].toarray(), dtype=np.float32))
    ctx.update_h()


def iteration(ctx):
    ctx.factorize(1, compute_w=True, compute_h=True, compute_err=False)


def kernel_ms(ctx, step, stem):
    ctx.profile_enable(True)
    step()
    st = ctx.kernel_stats()
    each = ctx.kernel_launch_ms()
    ctx.profile_enable(False)
    assert st["name"].startswith(stem) and len(each) == 1, (st, len(each))
    return float(each[0]), st


def big_shape(V, name):
    m, n = V.shape
    before = free_bytes()
    ctx = _lib.Context(ALGOS[name], m, n, K)
    try:
        upload_ms, _ = timed_ms(lambda: ctx.set_v_csr(V.indptr, V.indices, V.data))
        assert ctx.path_name == "cluster_csr"
        start(ctx, V, 2)
        iteration(ctx)                                            # warm-up
        device_bytes = before - free_bytes()
        it_ms, h_ms, w_ms = [], [], []
        rec = {}
        for _ in range(RUNS):
            it_ms.append(timed_ms(lambda: iteration(ctx))[0])
            a, rec["assign"] = kernel_ms(ctx, ctx.update_h, "k_cluster_csr_assign")
            b, rec["num"] = kernel_ms(ctx, ctx.update_w, "k_cluster_csr_num")
            h_ms.append(a)
            w_ms.append(b)
        ferr_ms, ferr = timed_ms(ctx.frobenius)
        res = {"shape": [m, n, K], "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "set_v_csr_ms": upload_ms,
               "device_bytes": device_bytes, "dense_image_bytes": 4 * m * n, "iteration_call_ms": stats(it_ms),
               "k_cluster_csr_assign_ms": stats(h_ms), "k_cluster_csr_num_ms": stats(w_ms), "frobenius_call_ms": ferr_ms,
               "ferr_over_norm": ferr / float(np.sqrt(np.sum(V.data.astype(np.float64) ** 2)))}
        for key, st in rec.items():
            res[key + "_record"] = {"name": st["name"], "flops": st["flops_per_launch"], "bytes": st["bytes_per_launch"]}
            ms = res["k_cluster_csr_%s_ms" % key]["median"]
            res[key + "_record"]["tb_per_s"] = st["bytes_per_launch"] / (ms * 1e-3) / 1e12
        return res
    finally:
        ctx.close()


def yardstick(V, name):
    m, n = V.shape
    ctxs = {"dense": _lib.Context(ALGOS[name], m, n, K), "sparse": _lib.Context(ALGOS[name], m, n, K)}
    try:
        ctxs["dense"].set_v_dense(V.toarray())
        ctxs["sparse"].set_v_csr(V.indptr, V.indices, V.data)
        paths = {label: ctx.path_name for label, ctx in ctxs.items()}
        for ctx in ctxs.values():
            start(ctx, V, 4)
        it = {label: [] for label in ctxs}
        kern = {"dense_pass": [], "sparse_assign": [], "sparse_num": []}
        for run in range(RUNS + 1):                              # run 0: warm-up, not recorded
            for label, ctx in ctxs.items():
                a = timed_ms(lambda: iteration(ctx))[0]
                if label == "dense":
                    k = {"dense_pass": kernel_ms(ctx, ctx.update_h, "k_cluster_pass")[0]}
                else:
                    k = {"sparse_assign": kernel_ms(ctx, ctx.update_h, "k_cluster_csr_assign")[0],
                         "sparse_num": kernel_ms(ctx, ctx.update_w, "k_cluster_csr_num")[0]}
                if run:
                    it[label].append(a)
                    for key, v in k.items():
                        kern[key].append(v)
        res = {"shape": [m, n, K], "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "paths": paths,
               "iteration_call_ms": {label: stats(v) for label, v in it.items()}, "kernel_ms": {key: stats(v) for key, v in kern.items()}}
        res["iteration_call_ms"]["dense_over_sparse"] = res["iteration_call_ms"]["dense"]["median"] / res["iteration_call_ms"]["sparse"]["median"]
        pair = res["kernel_ms"]["sparse_assign"]["median"] + res["kernel_ms"]["sparse_num"]["median"]
        res["kernel_ms"]["dense_pass_over_sparse_pair"] = res["kernel_ms"]["dense_pass"]["median"] / pair
        if name == "kmeans":
            res["assignments_equal"] = bool(np.array_equal(ctxs["dense"].get_assigned(), ctxs["sparse"].get_assigned()))
        return res
    finally:
        for ctx in ctxs.values():
            ctx.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--small"]
    small = "--small" in sys.argv[1:]
    part = args[0] if args else "large"
    out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "cluster_csr_bench.json")
    shift = 6 if small else 0
    try:
        with open(out_path) as f:
            res = json.load(f)
    except (OSError, ValueError):
        res = {}
    res.update({"runs": RUNS, "small": small})
    if part == "large":
        V = poisson_csr(1 << 14, (1 << 20) >> shift, 1e-3, 1)
        res["large"] = {name: big_shape(V, name) for name in ALGOS}
    elif part == "yardstick":
        V = poisson_csr(1 << 14, (1 << 15) >> shift, 1e-3, 3)
        res["yardstick"] = {name: yardstick(V, name) for name in ALGOS}
    else:
        raise SystemExit("part: large or yardstick")
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res[part], sort_keys=True))


if __name__ == "__main__":
    main()
