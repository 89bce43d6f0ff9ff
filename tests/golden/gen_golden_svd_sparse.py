"""Writes tests/golden/svd_sparse_tolerances.json: the deviation of the NumPy twin of the sparse SVD / PCA device path from the
float64 oracle, per quantity (tests/svd_sparse_cases.py: measure).  tests/test_svd_sparse_cases.py checks the file against a fresh
measurement.  The reference's own sparse branch (svd.py:160-244, eigsh) is not run here: no golden of it is stored, the oracle on
toarray() is the yardstick alone.

    python tests/golden/gen_golden_svd_sparse.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import svd_sparse_cases as sc   # noqa: E402

if __name__ == "__main__":
    out = dict(factor=sc.FACTOR, vector_floor=sc.VECTOR_FLOOR, ferr2_floor=sc.FERR2_FLOOR, measured=sc.measure(),
               cases=sorted(sc.SVD_CASES) + sorted(sc.PCA_CASES))
    with open(sc.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["measured"], indent=1, sort_keys=True))
