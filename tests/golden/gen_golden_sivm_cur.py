#!/usr/bin/env python3
"""Generate the SIVM_CUR golden vectors (tests/golden/sivmcur_*.npz) by running the REAL reference pymf/sivm_cur.py, imported
unmodified through the shim of gen_golden.py (pymf/sivm.py behind it through gen_golden_sivm.load_sivm: SIVM_CUR never reaches
the cvxopt stand-in, its SIVM objects run with compute_h=False), on the docstring case and on cases of tests/sivm_cur_cases.py.

dist.py:73-82 (cosine_distance) cannot run on dense data with more than one sample (gen_golden_sivm.py); for the cosine golden
the name `cosine_distance` that sivm.py imported is rebound, in the loaded module, to the formula it states for a single
vector, and the file says so (cosine_patched).  The reference is fed float64 arrays holding float32-representable values.  The
files hold data and results only."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden_sivm import cosine_single, load_sivm  # noqa: E402
import sivm_cur_cases as cc  # noqa: E402


def main():
    sivm = load_sivm()
    SIVM_CUR = importlib.import_module("pymf.sivm_cur").SIVM_CUR
    for name in cc.GOLDEN:
        rows, cols, rrank, _, _, _, metric, init = cc._spec(name)
        d = cc.data(name).astype(np.float64)
        patched = metric == "cosine"
        original = sivm.cosine_distance
        if patched:
            sivm.cosine_distance = cosine_single
        try:
            mdl = SIVM_CUR(d.copy(), rrank=rrank, dist_measure=metric, init=init)
            mdl.factorize()
        finally:
            sivm.cosine_distance = original
        out = dict(case=np.str_(name), rid=np.int64(mdl._rid), cid=np.int64(mdl._cid), U=np.asarray(mdl._U, dtype=np.float64),
                   ferr=np.float64(mdl.frobenius_norm()), cosine_patched=np.bool_(patched))
        if name == "doc_2x3":
            out["data"] = d
        np.savez_compressed(os.path.join(HERE, "sivmcur_" + name + ".npz"), **out)
        print("sivmcur_" + name, out["rid"], out["cid"], float(out["ferr"]))


if __name__ == "__main__":
    main()
