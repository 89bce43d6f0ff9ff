#!/usr/bin/env python3
"""Generate the CUR / CMD / pinv golden vectors (tests/golden/cur_*.npz, cmd_*.npz, pinv_*.npz) by running the REAL reference
pymf/cur.py, pymf/cmd.py and pymf/svd.py:pinv, imported unmodified through the shim of gen_golden.py, on the cases of
tests/cur_cases.py under np.random.seed, and write each case's condition numbers and the oracle-vs-twin deviation of the
error to tests/golden/cur_tolerances.json (rounded up to two digits; tests/test_cur_cases.py re-measures them and holds them
to the file).

The reference is fed float64 arrays holding float32-representable values.  C and R are not stored: they follow from the data
and the indices."""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import load_reference  # noqa: E402
from gen_golden_svd import round_up_2  # noqa: E402
import cur_cases as cc  # noqa: E402

PINV_CASES = {"20x30": (20, 30, 71), "300x40": (300, 40, 72)}   # name: (rows, cols, data seed), uniform float32 data


def pinv_data(name):
    rows, cols, seed = PINV_CASES[name]
    return np.random.RandomState(seed).rand(rows, cols).astype(np.float32)


def main():
    load_reference()
    mods = {"cur": importlib.import_module("pymf.cur").CUR, "cmd": importlib.import_module("pymf.cmd").CMD}
    svd = importlib.import_module("pymf.svd")
    for name, spec in cc.CUR_CASES.items():
        data = cc.data(name).astype(np.float64)
        for kind in cc.KINDS:
            np.random.seed(spec[5])
            mdl = mods[kind](data, rrank=spec[2])
            mdl.factorize()
            d = dict(case=np.str_(name), seed=np.int64(spec[5]), rrank=np.int64(spec[2]), rid=np.asarray(mdl._rid, dtype=np.int64),
                     cid=np.asarray(mdl._cid, dtype=np.int64), rcnt=np.asarray(mdl._rcnt, dtype=np.float64),
                     ccnt=np.asarray(mdl._ccnt, dtype=np.float64), U=np.asarray(mdl._U, dtype=np.float64),
                     ferr=np.float64(mdl.frobenius_norm()))
            np.savez_compressed(os.path.join(HERE, "%s_%s.npz" % (kind, name)), **d)
            print("%s_%-10s rows %3d cols %3d ferr %.6e" % (kind, name, len(d["rid"]), len(d["cid"]), d["ferr"]))
    for name, (rows, cols, seed) in PINV_CASES.items():
        A = pinv_data(name).astype(np.float64)
        P = np.asarray(svd.pinv(A.copy()))
        np.savez_compressed(os.path.join(HERE, "pinv_" + name + ".npz"), A_seed=np.int64(seed), A_shape=np.array([rows, cols], dtype=np.int64), P=P)
        print("pinv_%-8s %s" % (name, P.shape))
    cases = {k: {q: round_up_2(v) for q, v in fig.items()} for k, fig in cc.measure().items()}
    with open(cc.TOL_PATH, "w") as f:
        json.dump({"what": "per case of tests/cur_cases.py (cur_cases.measure): the condition numbers of the kept spectra of C^T C and "
                           "R R^T, tol_U = (kappa_c + kappa_r) x %g, and `ferr`, the deviation of the float32 twin's error from the "
                           "float64 oracle's relative to ||data||; all rounded up to two digits.  ferr_max is the largest `ferr`: the "
                           "device tolerance of the error is %g x that" % (cc.JACOBI_RTOL, cc.FACTOR),
                   "cases": cases, "ferr_max": max(fig["ferr"] for fig in cases.values())}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
