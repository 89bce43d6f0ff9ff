#!/usr/bin/env python3
"""CHNMF at 64 x 1 048 576 on one MI355X, base_sel 3 and 8 (3 and 28 pairs): the device hull pass pmf_chnmf_hull -- projection,
then per pair the filter sweeps and the chain, then the union -- and the whole CHNMF.update_w (the hull pass, the nested AA of
50 iterations on data[:, _hull_idx] and _map_w_to_data on the host), five runs each behind a warm-up call, alternating in one
process with k_sivm_pass<l2> on the same data (HIP events around every launch of a SIVM update_w): that pass reads the same
bytes once and is the yardstick.  The hull pass has no profile site of its own: the projection, one filter pair and one chain
alone are recorded as "not measured"; per pair the figure given is (hull pass of 28 pairs - hull pass of 3 pairs) / 25.
Writes profiles/chnmf_bench.json (or the path given as the first argument)."""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pymf_amd  # noqa: E402
from pymf_amd import _lib  # noqa: E402

M, N, K, REPS = 64, 1 << 20, 4, 5
SELS = (3, 8)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def main():
    warnings.simplefilter("ignore")
    rs = np.random.RandomState(0)
    V = np.empty((M, N), dtype=np.float32)
    for c0 in range(0, N, 1 << 16):
        V[:, c0:c0 + (1 << 16)] = rs.random_sample((M, 1 << 16))
    ctx = _lib.Context(_lib.ALGO_AA, M, N, K)
    ctx.set_v_dense(V)
    sivm = _lib.Context(_lib.ALGO_SIVM, M, N, K)
    sivm.set_v_dense(V)
    R = {s: np.random.RandomState(s).randn(s, M) for s in SELS}
    mdl = {s: pymf_amd.CHNMF(V, num_bases=K, base_sel=s) for s in SELS}
    hull_ms = {s: [] for s in SELS}
    upd_ms = {s: [] for s in SELS}
    upd_err = {}
    npts = {}
    pass_us = []
    for rep in range(REPS + 1):                                # (the first round is the warm-up)
        for s in SELS:
            t = ms(lambda: npts.__setitem__(s, int(ctx.chnmf_hull(R[s]).shape[0])))
            if rep:
                hull_ms[s].append(t)
        sivm.profile_enable(True)
        sivm.update_w()
        st = sivm.kernel_stats()
        sivm.profile_enable(False)
        if rep:
            pass_us.append(st["mean_ms"] * 1e3)
        for s in SELS:
            if s in upd_err:
                continue
            try:
                np.random.seed(100 + s)
                t = ms(mdl[s].update_w)
                if rep:
                    upd_ms[s].append(t)
            except Exception as e:                             # (the nested AA may refuse a start: recorded, not hidden)
                upd_err[s] = "%s: %s" % (type(e).__name__, e)
    y = float(np.median(pass_us))
    out = {"shape": [M, N], "num_bases": K, "reps": REPS, "yardstick_k_sivm_pass_l2_us": stats(pass_us), "yardstick_kernel": st["name"],
           "projection_us": "not measured", "one_filter_pair_us": "not measured", "one_chain_us": "not measured"}
    for s in SELS:
        h = stats(hull_ms[s])
        out["base_sel_%d" % s] = {
            "pairs": s * (s - 1) // 2, "hull_points": npts[s], "hull_pass_ms": h, "hull_pass_over_k_sivm_pass": h[0] * 1e3 / y,
            "update_w_ms": stats(upd_ms[s]) if upd_ms[s] and s not in upd_err else "not measured",
            "update_w_error": upd_err.get(s)}
    a, b = out["base_sel_%d" % SELS[0]], out["base_sel_%d" % SELS[1]]
    per_pair = (b["hull_pass_ms"][0] - a["hull_pass_ms"][0]) * 1e3 / (b["pairs"] - a["pairs"])
    out["per_pair_us_from_the_difference"] = per_pair
    out["per_pair_over_k_sivm_pass"] = per_pair / y
    print(json.dumps(out))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chnmf_bench.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
