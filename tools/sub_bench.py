#!/usr/bin/env python3
"""The column gather at 64 x 1 048 576 on one MI355X, nsel = 64, 1024 and 16 384 sorted random columns plus the whole copy,
beside the host path it replaces, in the same process: five runs behind one warm-up run, within each run every width in turn
and, per width, the two paths alternating.
  kernel   k_gather_cols alone: the profile site ("profile_gather"), an event pair around the launch
  call     pmf_set_v_gather_f32 followed by a synchronise of the destination (host clock)
  host     np.ascontiguousarray(data[:, idx]) + pmf_set_v_dense_f32 + synchronise (host clock); for the whole copy a second
           host upload of the full data
The yardstick is the host path on the same commit.  Achieved bytes per second of the kernel are on its algorithmic bytes:
4 m nsel read, 4 m nsel written, 4 nsel of indices (none for the whole copy).  Reports median and range over the five runs and
says per width whether the call beat the host path.  Writes profiles/sub_bench.json (or the path given as the first argument)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pymf_amd import _lib  # noqa: E402

M, N, RUNS = 64, 1 << 20, 5
NSELS = (64, 1024, 16384, None)                      # None: the whole copy


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)),
            "range": float(max(values) - min(values))}


def wall_ms(call, ctx):
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sub_bench.json")
    rs = np.random.RandomState(0)
    V = np.empty((M, N), dtype=np.float32)
    for c0 in range(0, N, 1 << 16):
        V[:, c0:c0 + (1 << 16)] = rs.random_sample((M, 1 << 16))
    src = _lib.Context(_lib.ALGO_CUR, M, N, 1)
    src.set_v_dense(V)
    src.synchronize()
    res = {"shape": [M, N], "runs": RUNS, "cases": {}}
    for nsel in NSELS:
        key = "whole_copy" if nsel is None else "nsel%d" % nsel
        idx = None if nsel is None else np.sort(rs.choice(N, nsel, replace=False)).astype(np.int64)
        cols = N if nsel is None else nsel
        dst = _lib.Context(_lib.ALGO_CUR, M, cols, 1)
        host = _lib.Context(_lib.ALGO_CUR, M, cols, 1)
        dst.set_option("profile_gather", 1)
        kernel_ms, call_ms, host_ms = [], [], []
        kname = ""
        for run in range(RUNS + 1):                  # run 0: warm-up, not recorded
            dst.profile_enable(True)
            c = wall_ms(lambda: dst.set_v_gather(src, idx), dst)
            st = dst.kernel_stats()
            dst.profile_enable(False)
            assert st["launches"] == 1 and st["name"].startswith("k_gather_cols"), st
            kname = st["name"]
            h = wall_ms(lambda: host.set_v_dense(V if idx is None else np.ascontiguousarray(V[:, idx])), host)
            if run:
                kernel_ms.append(st["mean_ms"])
                call_ms.append(c)
                host_ms.append(h)
        got = dst.get_v_dense()
        assert np.array_equal(got.view(np.uint32), (V if idx is None else V[:, idx]).view(np.uint32))
        alg_bytes = 8.0 * M * cols + (0.0 if idx is None else 4.0 * cols)
        k, c, h = stats(kernel_ms), stats(call_ms), stats(host_ms)
        res["cases"][key] = {"kernel": kname, "kernel_ms": k, "call_ms": c, "host_path_ms": h, "algorithmic_bytes": alg_bytes,
                             "kernel_GBps_on_algorithmic_bytes": alg_bytes / (k["median"] * 1e-3) / 1e9,
                             "call_over_host_path": c["median"] / h["median"],
                             "call_beats_host_path": bool(c["median"] < h["median"])}
        dst.close()
        host.close()
    src.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
