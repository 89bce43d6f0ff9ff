#!/usr/bin/env python3
"""SIVM_GSAT at 64 x 1 048 576, k = 64 on one MI355X: a walk of 10 000 probes from a SIVM_SGREEDY selection and from the init_w
start (the first 64 columns), the two alternating in one process, five runs each behind one warm-up run.  Every run starts
from the same vertices and walks the same seeded indices.  Reports, as median and range over the runs, the wall time of the
pmf_gsat_walk call per probe, and per start the number of swaps, of skipped probes and of launch pairs per 256-probe batch
(from the verdicts: one pair per batch and one more behind every accepted probe that is not the last of its batch).
The yardstick the design names for one float64 elimination of this size, k_sgreedy_step at t = 63, has no profile site of its
own and is not timed here.  Writes profiles/gsat_bench.json (or the path given)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

M, N, K, RUNS, PROBES, BATCH = 64, 1 << 20, 64, 5, 10000, 256


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)),
            "range": float(max(values) - min(values))}


def launch_pairs(slots):
    count = 0
    for base in range(0, len(slots), BATCH):
        part = slots[base:base + BATCH]
        off = 0
        while off < len(part):
            count += 1
            acc = np.nonzero(part[off:] >= 0)[0]
            off = len(part) if len(acc) == 0 else off + int(acc[0]) + 1
    return count


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gsat_bench.json")
    rs = np.random.RandomState(0)                    # the data of tools/sgreedy_bench.py
    verts = 4.0 * np.linspace(1.0, 3.0, K) * np.linalg.qr(rs.randn(M, M))[0][:, :K]
    V = np.empty((M, N), dtype=np.float32)
    for c0 in range(0, N, 1 << 16):
        h = 0.8 * rs.dirichlet(np.full(K, 0.5), size=1 << 16).T + 0.2 / K
        V[:, c0:c0 + (1 << 16)] = verts.dot(h) + 0.12 * rs.randn(M, 1 << 16) / 8.0
    cols = rs.choice(N, K, replace=False)
    V[:, cols] = verts
    idx = np.floor(np.random.RandomState(1).random_sample(PROBES) * N).astype(np.int64)

    sg = _lib.Context(_lib.ALGO_SIVM, M, N, K)
    sg.set_v_dense(V)
    sg.set_option("sivm_sgreedy", 1)
    sg.update_w()
    starts = {"sgreedy": [int(s) for s in sg.get_select()], "init_w": list(range(K))}
    sg.close()

    ctx = _lib.Context(_lib.ALGO_SIVM, M, N, K)
    ctx.set_v_dense(V)
    ctx.set_option("sivm_gsat", 1)
    per_probe = {label: [] for label in starts}
    facts = {}
    for run in range(RUNS + 1):                      # run 0: warm-up, not recorded
        for label, select in starts.items():
            ctx.set_w(np.ascontiguousarray(V[:, select]))
            ctx.gsat_start(select, force=True)
            v0 = ctx.gsat_get_volumes()[1]
            ctx.synchronize()
            t0 = time.perf_counter()
            slots = ctx.gsat_walk(idx)
            ms = (time.perf_counter() - t0) * 1e3
            if run == 0:
                pairs = launch_pairs(slots)
                facts[label] = {"swaps": int((slots >= 0).sum()), "skipped": int((slots == -2).sum()), "launch_pairs": pairs,
                                "launch_pairs_per_batch": pairs / float(-(-PROBES // BATCH)), "volume_before": v0,
                                "volume_after": ctx.gsat_get_volumes()[1]}
                continue
            per_probe[label].append(ms * 1e3 / PROBES)
    ctx.close()
    res = {"shape": [M, N, K], "probes": PROBES, "runs": RUNS, "walk_us_per_probe": {label: stats(v) for label, v in per_probe.items()},
           "walk": facts, "k_sgreedy_step_t63": "not timed: the kernel has no profile site"}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
