#!/usr/bin/env python3
"""Writes tests/golden/cluster_sparse_tolerances.json: the deviation of the float64 trace identity from the direct error on the
oracle's Kmeans and Cmeans factors, relative to ||data||, per case of tests/cluster_sparse_cases.py (measure), rounded up to two
digits; tests/test_cluster_sparse_cases.py checks the file against a fresh measurement.  The reference has no sparse clustering
branch, so there is nothing of its own to record.

    python tests/golden/gen_golden_cluster_sparse.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cluster_sparse_cases as cs   # noqa: E402


if __name__ == "__main__":
    fresh = cs.measure()
    measured = {name: {key: (cs.round_up_2(v) if key in ("kmeans", "cmeans") else round(v, 4)) for key, v in row.items()}
                for name, row in fresh.items()}
    out = dict(factor=cs.FACTOR, measured=measured, ferr_max=max(max(v["kmeans"], v["cmeans"]) for v in measured.values()),
               cases=sorted(measured))
    with open(cs.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
