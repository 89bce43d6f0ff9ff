#!/usr/bin/env python3
"""CUR on CSR data (k_cur_csr_sqnorms, k_cur_csr_gather, k_cur_csr_mid; pmf_cur_csr.h) on one MI355X.

(a) 1 048 576 x 16 384 at 0.1 % stored entries, rrank = 64 (64 rows and 64 columns drawn by their squared norms, sorted, as
    CUR.sample draws them): behind one warm-up call each, five runs of the pmf_cur_sqnorms call and of the pmf_cur_compute call
    (host wall clock around the call, which returns with the device idle: downloads, the two Jacobi solves and the host finish
    are in it), and of k_cur_csr_mid alone (pmf_profile_enable's event pair around its launch).
(b) The yardstick, 65 536 x 4 096 at 1 % stored entries, rrank = 64: the dense path on toarray() and the sparse path on the
    same matrix with the same indices, in one process, alternating within each of five runs behind one warm-up run; both calls.
Writes profiles/cur_csr_bench.json (or the path given).  `--small` runs both parts at 1/64 of the rows (a plumbing check)."""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

RUNS, RRANK = 5, 64


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)),
            "range": float(max(values) - min(values))}


def poisson_csr(m, n, density, seed):
    """A canonical float32 csr_matrix whose rows hold about Poisson(density n) entries at uniform columns (a column drawn twice
    is kept once), values in [0.25, 1.25)."""
    rs = np.random.RandomState(seed)
    counts = rs.poisson(density * n, size=m).astype(np.int64)
    key = np.unique(np.repeat(np.arange(m, dtype=np.int64), counts) * n + rs.randint(0, n, size=int(counts.sum())))
    indptr = np.searchsorted(key, np.arange(m + 1, dtype=np.int64) * n).astype(np.int64)
    vals = (rs.random_sample(key.shape[0]) + 0.25).astype(np.float32)
    return sp.csr_matrix((vals, (key % n).astype(np.int32), indptr), shape=(m, n))


def timed_ms(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def draw(ctx, seed):
    row_sq, col_sq = ctx.cur_sqnorms()
    rs = np.random.RandomState(seed)
    rid = np.sort(rs.choice(row_sq.shape[0], RRANK, p=row_sq / row_sq.sum())).astype(np.int32)
    cid = np.sort(rs.choice(col_sq.shape[0], RRANK, p=col_sq / col_sq.sum())).astype(np.int32)
    return rid, cid


def big_shape(V):
    m, n = V.shape
    ctx = _lib.Context(_lib.ALGO_CUR, m, n, RRANK)
    try:
        upload_ms, _ = timed_ms(lambda: ctx.set_v_csr(V.indptr, V.indices, V.data))
        assert ctx.path_name == "cur_csr"
        rid, cid = draw(ctx, 5)                                   # (the warm-up of pmf_cur_sqnorms)
        ones = np.ones(RRANK, dtype=np.int32)
        ctx.cur_compute(rid, ones, cid, ones)                     # warm-up
        sq_ms, cp_ms, mid_ms = [], [], []
        for _ in range(RUNS):
            sq_ms.append(timed_ms(ctx.cur_sqnorms)[0])
            cp_ms.append(timed_ms(lambda: ctx.cur_compute(rid, ones, cid, ones))[0])
            ctx.set_option("profile_cur", 0)
            ctx.profile_enable(True)
            ctx.cur_compute(rid, ones, cid, ones)
            st = ctx.kernel_stats()
            each = ctx.kernel_launch_ms()
            ctx.profile_enable(False)
            assert st["name"].startswith("k_cur_csr_mid") and len(each) == 1, (st, len(each))
            mid_ms.append(float(each[0]))
        return {"shape": [m, n, RRANK], "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "kernel": st["name"],
                "set_v_csr_ms": upload_ms, "cur_sqnorms_call_ms": stats(sq_ms), "cur_compute_call_ms": stats(cp_ms),
                "k_cur_csr_mid_ms": stats(mid_ms), "ferr_over_norm": ctx.cur_ferr() / float(np.sqrt(np.sum(V.data.astype(np.float64) ** 2)))}
    finally:
        ctx.close()


def yardstick(V):
    m, n = V.shape
    ctxs = {"dense": _lib.Context(_lib.ALGO_CUR, m, n, RRANK), "sparse": _lib.Context(_lib.ALGO_CUR, m, n, RRANK)}
    try:
        ctxs["dense"].set_v_dense(V.toarray())
        ctxs["sparse"].set_v_csr(V.indptr, V.indices, V.data)
        paths = {label: ctx.path_name for label, ctx in ctxs.items()}
        rid, cid = draw(ctxs["sparse"], 6)
        ones = np.ones(RRANK, dtype=np.int32)
        sq = {label: [] for label in ctxs}
        cp = {label: [] for label in ctxs}
        for run in range(RUNS + 1):                              # run 0: warm-up, not recorded
            for label, ctx in ctxs.items():
                a = timed_ms(ctx.cur_sqnorms)[0]
                b = timed_ms(lambda: ctx.cur_compute(rid, ones, cid, ones))[0]
                if run:
                    sq[label].append(a)
                    cp[label].append(b)
        Ud, Us = ctxs["dense"].cur_get(want="U")[1], ctxs["sparse"].cur_get(want="U")[1]
        res = {"shape": [m, n, RRANK], "nnz": int(V.nnz), "density": V.nnz / float(m) / n, "paths": paths,
               "cur_sqnorms_call_ms": {label: stats(v) for label, v in sq.items()},
               "cur_compute_call_ms": {label: stats(v) for label, v in cp.items()},
               "U_sparse_vs_dense_rel_max": float(np.max(np.abs(Us - Ud)) / np.max(np.abs(Ud)))}
        for key in ("cur_sqnorms_call_ms", "cur_compute_call_ms"):
            res[key]["dense_over_sparse"] = res[key]["dense"]["median"] / res[key]["sparse"]["median"]
        return res
    finally:
        for ctx in ctxs.values():
            ctx.close()


def main():
    args = [a for a in sys.argv[1:] if a != "--small"]
    small = "--small" in sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "cur_csr_bench.json")
    shift = 6 if small else 0
    res = {"runs": RUNS, "small": small,
           "large": big_shape(poisson_csr((1 << 20) >> shift, 1 << 14, 1e-3, 1)),
           "yardstick": yardstick(poisson_csr((1 << 16) >> shift, 1 << 12, 1e-2, 3))}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
