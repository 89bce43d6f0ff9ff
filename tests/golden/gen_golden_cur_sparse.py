#!/usr/bin/env python3
"""Write tests/golden/cur_sparse_tolerances.json: per case of tests/cur_sparse_cases.py the condition numbers, tol_U, the
deviation of the trace identity's error from the direct one (both NumPy float64 on the oracle's matrices, relative to
||data||) and ferr / ||data||, rounded up to two digits; tests/test_cur_sparse_cases.py re-measures them and holds them to
the file.  No reference run is involved: the yardstick of the sparse path is the float64 oracle on toarray()."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden_svd import round_up_2  # noqa: E402
import cur_cases as cc  # noqa: E402
import cur_sparse_cases as scs  # noqa: E402


def main():
    cases = {k: {q: round_up_2(v) for q, v in fig.items()} for k, fig in scs.measure().items()}
    with open(scs.TOL_PATH, "w") as f:
        json.dump({"what": "per case of tests/cur_sparse_cases.py (measure): the condition numbers of the kept spectra of C^T C and "
                           "R R^T, tol_U = (kappa_c + kappa_r) x %g, `ferr`, the deviation of the trace identity's error from the direct "
                           "one relative to ||data||, and ferr_rel = ferr / ||data||; all rounded up to two digits.  ferr_max is the "
                           "largest `ferr`: the device tolerance of frobenius_norm is %g x that, floored at %g.  ferr_dense is the deviation of "
                           "the dense path's float32 twin (cur_oracle.twin) from the oracle, ferr_dense_max its largest"
                           % (cc.JACOBI_RTOL, cc.FACTOR, scs.FERR_FLOOR),
                   "cases": cases, "ferr_max": max(fig["ferr"] for fig in cases.values()),
                   "ferr_dense_max": max(fig["ferr_dense"] for fig in cases.values())}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("ferr_max %.3e -> device tolerance %.3e" % (max(fig["ferr"] for fig in cases.values()), scs.device_tol_ferr()))


if __name__ == "__main__":
    main()
