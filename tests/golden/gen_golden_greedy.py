#!/usr/bin/env python3
"""Generate the GREEDY / GREEDYCUR golden vectors (tests/golden/greedy_*.npz, greedycur_*.npz) by running the REAL reference
pymf/greedy.py and pymf/greedycur.py, imported unmodified through the shim of gen_golden.py (they need only svd, nmf and cur:
no cvxopt stand-in), on the docstring cases and on cases of tests/greedy_cases.py.

The reference is fed float64 arrays holding float32-representable values.  The files hold data and results only."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import load_reference  # noqa: E402
import greedy_cases as gc  # noqa: E402

DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])             # greedy.py:57
DOC_USERW = (np.array([[1.5, 1.3], [1.2, 0.3]]), np.array([[1.0, 0.0], [0.0, 1.0]]))   # greedy.py:65-66
CASES = ("29x300_k6", "300x29_k6", "37x29_k5")
CUR_CASES = ("40x300", "300x40")


def save(name, **d):
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
    print(name, {k: np.asarray(v).shape for k, v in d.items()})


def run(GREEDY, data, k, **kw):
    np.random.seed(1)
    mdl = GREEDY(data, num_bases=k)
    mdl.factorize(**kw)
    return mdl


def main():
    load_reference()
    GREEDY = importlib.import_module("pymf.greedy").GREEDY
    GREEDYCUR = importlib.import_module("pymf.greedycur").GREEDYCUR
    mdl = run(GREEDY, DOC.copy(), 2, niter=10)
    save("greedy_doc_2x3", data=DOC, select=np.int64(mdl.select), W=mdl.W, H=mdl.H, ferr=mdl.ferr)
    data, W = DOC_USERW
    mdl = GREEDY(data.copy(), num_bases=2)
    mdl.W = W.copy()
    mdl.factorize(compute_w=False)
    save("greedy_doc_userw", data=data, W=W, H=mdl.H, ferr=np.float64(mdl.ferr[0]))
    for name in CASES:
        d = gc.data(name).astype(np.float64)
        k = (gc.GREEDY_CASES.get(name) or gc.GOLDEN_ONLY[name])[2]
        mdl = run(GREEDY, d.copy(), k)
        save("greedy_" + name, case=np.str_(name), select=np.int64(mdl.select), H=mdl.H, ferr=np.float64(mdl.ferr[0]))
    d = gc.data("29x300_k6").astype(np.float64)
    mdl = run(GREEDY, d.copy(), 6, niter=3)
    save("greedy_29x300_k6_niter3", case=np.str_("29x300_k6"), select=np.int64(mdl.select), ferr=mdl.ferr)
    for name in CUR_CASES:
        d = gc.data(name).astype(np.float64)
        mdl = GREEDYCUR(d.copy(), rrank=gc.GREEDYCUR_CASES[name][2])
        mdl.factorize()
        save("greedycur_" + name, case=np.str_(name), rid=np.int64(mdl._rid), cid=np.int64(mdl._cid), U=np.asarray(mdl._U, dtype=np.float64),
             ferr=np.float64(mdl.frobenius_norm()))


if __name__ == "__main__":
    main()
