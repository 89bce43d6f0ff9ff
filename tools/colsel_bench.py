#!/usr/bin/env python3
"""LAESA and GMAP at 64 x 1 048 576, k = 64 on one MI355X beside SIVM on the same data in the same process: five runs, the
four contexts alternating within each run (LAESA l2, GMAP pca, SIVM l2, SIVM cosine), behind one warm-up run.  Per run and
context one unprofiled update_w for the call's wall time and one profiled update_w for the per-launch times of its pass
kernel (event pairs around every launch); per-pass figure = mean over the launches of the run (GMAP: over rounds >= 1, round
0 reads no x and is reported on its own).  Reports median and range over the five runs and the condition of DESIGN.md 3.19:
the median of k_laesa_pass<l2> is not above that of k_sivm_pass<l2> by more than the range k_sivm_pass<l2> itself shows,
likewise k_gmap_pass<pca> against k_sivm_pass<cosine>.  Writes profiles/colsel_bench.json (or the path given)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

M, N, K, RUNS = 64, 1 << 20, 64, 5


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)),
            "range": float(max(values) - min(values))}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "colsel_bench.json")
    rs = np.random.RandomState(0)                    # the data of tools/sivm_bench.py
    verts = 4.0 * np.linspace(1.0, 3.0, K) * np.linalg.qr(rs.randn(M, M))[0][:, :K]
    V = np.empty((M, N), dtype=np.float32)
    for c0 in range(0, N, 1 << 16):
        h = 0.8 * rs.dirichlet(np.full(K, 0.5), size=1 << 16).T + 0.2 / K
        V[:, c0:c0 + (1 << 16)] = verts.dot(h) + 0.12 * rs.randn(M, 1 << 16) / 8.0
    V[:, rs.choice(N, K, replace=False)] = verts

    # label: (sivm_rule, sivm_metric / gmap_method, kernel name, launches to average from)
    specs = {"laesa_l2": (1, 0, "k_laesa_pass<l2>", 0), "gmap_pca": (2, 0, "k_gmap_pass<pca>", 1),
             "sivm_l2": (0, 0, "k_sivm_pass<l2>", 0), "sivm_cosine": (0, 2, "k_sivm_pass<cosine>", 0)}
    ctxs = {}
    for label, (rule, what, _, _) in specs.items():
        ctx = _lib.Context(_lib.ALGO_SIVM, M, N, K)
        ctx.set_v_dense(V)
        ctx.set_option("sivm_rule", rule)
        ctx.set_option("gmap_method" if rule == 2 else "sivm_metric", what)
        ctxs[label] = ctx
    wall = {label: [] for label in specs}
    per_pass = {label: [] for label in specs}
    round0 = []
    launches = {}
    for run in range(RUNS + 1):                      # run 0: warm-up, not recorded
        for label, (_, _, kernel, first) in specs.items():
            ctx = ctxs[label]
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.update_w()
            ctx.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            ctx.profile_enable(True)
            ctx.update_w()
            st = ctx.kernel_stats()
            each = ctx.kernel_launch_ms()
            ctx.profile_enable(False)
            assert st["name"] == kernel and len(each) == st["launches"], (st, len(each))
            if run == 0:
                launches[label] = {"kernel": kernel, "launches": int(st["launches"]), "bytes_per_launch": st["bytes_per_launch"]}
                continue
            wall[label].append(ms)
            per_pass[label].append(float(np.mean(each[first:])))
            if label == "gmap_pca":
                round0.append(float(each[0]))
    res = {"shape": [M, N, K], "runs": RUNS, "kernels": launches,
           "update_w_ms": {label: stats(v) for label, v in wall.items()},
           "per_pass_ms": {label: stats(v) for label, v in per_pass.items()},
           "k_gmap_pass_round0_ms": stats(round0)}
    for label in specs:
        res["per_pass_ms"][label]["TBps"] = launches[label]["bytes_per_launch"] / (res["per_pass_ms"][label]["median"] * 1e-3) / 1e12
    p = res["per_pass_ms"]
    res["condition"] = {
        "laesa_l2_vs_sivm_l2": bool(p["laesa_l2"]["median"] <= p["sivm_l2"]["median"] + p["sivm_l2"]["range"]),
        "gmap_pca_vs_sivm_cosine": bool(p["gmap_pca"]["median"] <= p["sivm_cosine"]["median"] + p["sivm_cosine"]["range"])}
    for ctx in ctxs.values():
        ctx.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
