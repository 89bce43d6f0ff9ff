#!/usr/bin/env python3
"""SIVM_SGREEDY at 64 x 1 048 576, k = 64 on one MI355X beside LAESA on the same data in the same process: five runs, the two
contexts alternating within each run, behind one warm-up run.  Per run and context one unprofiled update_w for the call's wall
time and one profiled update_w for the per-launch times of its pass kernel (event pairs around every launch).  Reports, as
median and range over the five runs, the update_w call of both, the mean k_laesa_pass<l2> launch, and k_sgreedy_pass at t = 1,
32 and 63 with the TB/s each reaches on its algorithmic bytes (4 m np + 4 np + 4 (t - 1) np) -- and the yardstick of DESIGN.md
3.20: the time those bytes would take at the bandwidth k_laesa_pass<l2> reaches in this run, and the ratio of the measured
time to it (above about 2 at t = 63: the float64 form is the limiter).  Writes profiles/sgreedy_bench.json (or the path
given)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

M, N, K, RUNS = 64, 1 << 20, 64, 5
ROUNDS = (1, 32, 63)


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)),
            "range": float(max(values) - min(values))}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sgreedy_bench.json")
    rs = np.random.RandomState(0)                    # the data of tools/sivm_bench.py and tools/colsel_bench.py
    verts = 4.0 * np.linspace(1.0, 3.0, K) * np.linalg.qr(rs.randn(M, M))[0][:, :K]
    V = np.empty((M, N), dtype=np.float32)
    for c0 in range(0, N, 1 << 16):
        h = 0.8 * rs.dirichlet(np.full(K, 0.5), size=1 << 16).T + 0.2 / K
        V[:, c0:c0 + (1 << 16)] = verts.dot(h) + 0.12 * rs.randn(M, 1 << 16) / 8.0
    cols = rs.choice(N, K, replace=False)
    V[:, cols] = verts

    specs = {"sgreedy": ("sivm_sgreedy", "k_sgreedy_pass"), "laesa_l2": ("sivm_rule", "k_laesa_pass<l2>")}
    ctxs = {}
    for label, (option, _) in specs.items():
        ctx = _lib.Context(_lib.ALGO_SIVM, M, N, K)
        ctx.set_v_dense(V)
        ctx.set_option(option, 1)
        ctxs[label] = ctx
    wall = {label: [] for label in specs}
    laesa_pass = []
    at_round = {t: [] for t in ROUNDS}
    launches = {}
    np_ = -(-N // 64) * 64
    for run in range(RUNS + 1):                      # run 0: warm-up, not recorded
        for label, (_, kernel) in specs.items():
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
            if label == "laesa_l2":
                laesa_pass.append(float(np.mean(each)))
            else:
                for t in ROUNDS:
                    at_round[t].append(float(each[t - 1]))
    res = {"shape": [M, N, K], "runs": RUNS, "kernels": launches,
           "update_w_ms": {label: stats(v) for label, v in wall.items()},
           "k_laesa_pass_l2_ms": stats(laesa_pass), "k_sgreedy_pass_ms": {}}
    laesa_bw = launches["laesa_l2"]["bytes_per_launch"] / (res["k_laesa_pass_l2_ms"]["median"] * 1e-3)
    res["k_laesa_pass_l2_ms"]["TBps"] = laesa_bw / 1e12
    for t in ROUNDS:
        s = stats(at_round[t])
        nbytes = 4.0 * M * np_ + 4.0 * np_ + 4.0 * (t - 1) * np_
        s["bytes"] = nbytes
        s["TBps"] = nbytes / (s["median"] * 1e-3) / 1e12
        s["ms_at_laesa_bandwidth"] = nbytes / laesa_bw * 1e3
        s["ratio_to_laesa_bandwidth"] = s["median"] / s["ms_at_laesa_bandwidth"]
        res["k_sgreedy_pass_ms"]["t=%d" % t] = s
    res["form_is_the_limiter_at_t63"] = bool(res["k_sgreedy_pass_ms"]["t=63"]["ratio_to_laesa_bandwidth"] > 2.0)
    sel = ctxs["sgreedy"].get_select().tolist()
    res["sgreedy_selects_the_planted_vertices"] = bool(sorted(sel) == sorted(int(c) for c in cols))
    for ctx in ctxs.values():
        ctx.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
