#!/usr/bin/env python3
"""Generate the CURSL golden vectors (tests/golden/cursl_*.npz) by running the REAL reference pymf/cursl.py, imported
unmodified through the shim of gen_golden.py, on the cases of tests/cursl_cases.py under np.random.seed, and write each
case's condition numbers, tol_cum and the oracle-vs-twin deviation of the error to tests/golden/cursl_tolerances.json
(rounded up to two digits; tests/test_cursl_cases.py re-measures them and holds them to the file).

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
import cursl_cases as csc  # noqa: E402


def main():
    load_reference()
    CURSL = importlib.import_module("pymf.cursl").CURSL
    for name, spec in csc.CURSL_CASES.items():
        data = csc.data(name).astype(np.float64)
        np.random.seed(spec[5])
        mdl = CURSL(data, rrank=spec[2])
        # factorize() as cmd.py:72-89 runs it, keeping the probabilities it draws from
        prow, pcol = mdl.sample_probability()
        mdl._rid = mdl.sample(mdl._rrank, prow)
        mdl._cid = mdl.sample(mdl._crank, pcol)
        mdl._cmdinit()
        mdl.computeUCR()
        d = dict(case=np.str_(name), seed=np.int64(spec[5]), rrank=np.int64(spec[2]), rid=np.asarray(mdl._rid, dtype=np.int64),
                 cid=np.asarray(mdl._cid, dtype=np.int64), rcnt=np.asarray(mdl._rcnt, dtype=np.float64),
                 ccnt=np.asarray(mdl._ccnt, dtype=np.float64), prow=np.asarray(prow, dtype=np.float64).ravel(),
                 pcol=np.asarray(pcol, dtype=np.float64).ravel(), U=np.asarray(mdl._U, dtype=np.float64),
                 ferr=np.float64(mdl.frobenius_norm()))
        # the same seed through factorize() itself gives the same draws
        np.random.seed(spec[5])
        again = CURSL(data, rrank=spec[2])
        again.factorize()
        assert np.array_equal(again._rid, mdl._rid) and np.array_equal(again._cid, mdl._cid)
        np.savez_compressed(os.path.join(HERE, "cursl_%s.npz" % name), **d)
        print("cursl_%-12s rows %3d cols %3d ferr %.6e" % (name, len(d["rid"]), len(d["cid"]), d["ferr"]))
    cases = {k: {q: round_up_2(v) for q, v in fig.items()} for k, fig in csc.measure().items()}
    with open(csc.TOL_PATH, "w") as f:
        json.dump({"what": "per case of tests/cursl_cases.py (cursl_cases.measure): the condition numbers of the kept spectra of C^T C "
                           "and R R^T, tol_U = (kappa_c + kappa_r) x %g, tol_cum = %g x (1 + lambda_kk / (lambda_kk - lambda_kk+1)), and "
                           "`ferr`, the deviation of the float32 twin's error from the float64 oracle's relative to ||data||; all "
                           "rounded up to two digits.  ferr_max is the largest `ferr`: the device tolerance of the error is %g x "
                           "that" % (cc.JACOBI_RTOL, cc.JACOBI_RTOL, cc.FACTOR),
                   "cases": cases, "ferr_max": max(fig["ferr"] for fig in cases.values())}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
