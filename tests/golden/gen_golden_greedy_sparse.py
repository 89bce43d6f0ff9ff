#!/usr/bin/env python3
"""Writes tests/golden/greedy_sparse_tolerances.json: the deviation of the float64 trace identity from the direct error on the
oracle's factors, per case of tests/greedy_sparse_cases.py (measure); tests/test_greedy_sparse_cases.py checks the file against a
fresh measurement.

With --reference it also tries the reference's own sparse branch (pymf/greedy.py:115-141 on a csc_matrix), imported unmodified
through the shim of gen_golden.py, on the two smallest cases, and records its `select` in tests/golden/greedy_sparse_<case>.npz
where it runs; what it prints otherwise is why it did not.

    python tests/golden/gen_golden_greedy_sparse.py [--reference]
"""
import json
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import greedy_sparse_cases as gs   # noqa: E402

REFERENCE_CASES = ("29x300_k6", "300x29_k6")


def reference_selects():
    import importlib
    from gen_golden import load_reference
    load_reference()
    GREEDY = importlib.import_module("pymf.greedy").GREEDY
    for name in REFERENCE_CASES:
        A = gs.matrix(name).astype(np.float64).tocsc()
        try:
            np.random.seed(1)
            mdl = GREEDY(A, num_bases=gs.num_bases(name))
            mdl.factorize(compute_h=False, compute_err=False)
        except Exception:
            print("%s: the reference's sparse branch did not run:" % name)
            traceback.print_exc()
            continue
        np.savez_compressed(os.path.join(HERE, "greedy_sparse_%s.npz" % name), case=np.str_(name), select=np.int64(mdl.select))
        print(name, "reference select", list(mdl.select), "oracle", gs.case(name)["select"])


if __name__ == "__main__":
    measured = gs.measure()
    out = dict(factor=gs.FACTOR, measured=measured, ferr_max=max(v["ferr"] for v in measured.values()), cases=sorted(measured))
    with open(gs.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    if "--reference" in sys.argv:
        reference_selects()
