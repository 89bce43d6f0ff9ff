#!/usr/bin/env python3
"""k_vq_pass at 64 x 1 048 576 on one MI355X, nq = 1, 16, 64 and 128 query vectors, both metrics, beside k_sivm_pass<l2> on the
same data in the same process: five runs behind one warm-up run, within each run the SIVM context and every (metric, nq) of
the vq context in turn.  Per run one profiled pmf_vq_columns call per (metric, nq) (an event pair around its k_vq_pass launch)
and one profiled SIVM update_w (event pairs around every k_sivm_pass<l2> launch, the mean over them).  The yardstick is the
single-column pass: ratio = k_vq_pass time / (nq x k_sivm_pass<l2> time); below 1 the sweep beats nq single-column passes.  Also
timed, nq = 16 and 128, l2: the assign direction (k_vq_pass writing the float64 block, and k_vq_argmin_rows).
Reports median and range over the five runs.  Writes profiles/vq_bench.json (or the path given as the first argument)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

M, N, K, RUNS = 64, 1 << 20, 4, 5
NQS = (1, 16, 64, 128)
METRICS = (("l2", 0), ("l1", 1))


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)),
            "range": float(max(values) - min(values))}


def timed(ctx, site, call):
    """mean ms of the launches of profile site `site` inside call(), and the site's name"""
    ctx.set_option("profile_vq", site)
    ctx.profile_enable(True)
    call()
    st = ctx.kernel_stats()
    ctx.profile_enable(False)
    ctx.set_option("profile_vq", 0)
    return st["mean_ms"], st["name"], st["launches"]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vq_bench.json")
    rs = np.random.RandomState(0)
    V = np.empty((M, N), dtype=np.float32)
    for c0 in range(0, N, 1 << 16):
        V[:, c0:c0 + (1 << 16)] = rs.random_sample((M, 1 << 16))
    Q = np.ascontiguousarray(V[:, rs.choice(N, max(NQS), replace=False)] + 0.01 * rs.standard_normal((M, max(NQS))), dtype=np.float32)
    ctx = _lib.Context(_lib.ALGO_SIVM, M, N, K)
    ctx.set_v_dense(V)
    sivm = _lib.Context(_lib.ALGO_SIVM, M, N, K)
    sivm.set_v_dense(V)
    vq_ms = {(name, nq): [] for name, _ in METRICS for nq in NQS}
    asg_ms = {nq: {"k_vq_pass<l2> want_all": [], "k_vq_argmin_rows": []} for nq in (16, 128)}
    sivm_ms = []
    names = {}
    for run in range(RUNS + 1):                      # run 0: warm-up, not recorded
        sivm.profile_enable(True)
        sivm.update_w()
        st = sivm.kernel_stats()
        sivm.profile_enable(False)
        assert st["name"] == "k_sivm_pass<l2>", st
        if run:
            sivm_ms.append(st["mean_ms"])
        for name, met in METRICS:
            for nq in NQS:
                ms, kname, launches = timed(ctx, 1, lambda: ctx.vq_columns(Q[:, :nq], met))
                assert kname == "k_vq_pass<%s>" % name and launches == 1, (kname, launches)
                names[name] = kname
                if run:
                    vq_ms[name, nq].append(ms)
        for nq in asg_ms:
            a, _, _ = timed(ctx, 1, lambda: ctx.vq_assign(Q[:, :nq], 0, want_idx=True, want_dist=False))
            b, kname, _ = timed(ctx, 2, lambda: ctx.vq_assign(Q[:, :nq], 0, want_idx=True, want_dist=False))
            assert kname == "k_vq_argmin_rows", kname
            if run:
                asg_ms[nq]["k_vq_pass<l2> want_all"].append(a)
                asg_ms[nq]["k_vq_argmin_rows"].append(b)
    y = stats(sivm_ms)
    res = {"shape": [M, N], "runs": RUNS, "yardstick_k_sivm_pass_l2_ms": y, "k_vq_pass_ms": {}, "ratio_vq_over_nq_sivm_passes": {},
           "assign_direction_ms": {str(nq): {k: stats(v) for k, v in d.items()} for nq, d in asg_ms.items()}}
    for (name, nq), v in sorted(vq_ms.items()):
        s = stats(v)
        s["Tflops_3mn_nq"] = 3.0 * M * N * nq / (s["median"] * 1e-3) / 1e12
        res["k_vq_pass_ms"]["%s_nq%d" % (name, nq)] = s
        res["ratio_vq_over_nq_sivm_passes"]["%s_nq%d" % (name, nq)] = s["median"] / (nq * y["median"])
    res["sweep_beats_nq_single_passes_at_nq64"] = {name: bool(res["ratio_vq_over_nq_sivm_passes"]["%s_nq64" % name] < 1.0) for name, _ in METRICS}
    ctx.close()
    sivm.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
