#!/usr/bin/env python3
"""Generate the SIVM_SGREEDY golden vectors (tests/golden/sgreedy_*.npz) by running the REAL reference pymf/sivm_sgreedy.py
(with sivm_search.py, sivm.py, aa.py, vol.py and dist.py behind it), imported unmodified through the shims of gen_golden.py and
gen_golden_sivm.py (the cvxopt stand-in: H and ferr pin aa.py's data flow, not cvxopt's digits).

Two names that vol.py and sivm_search.py import no longer exist in a current SciPy; stand-ins are installed BEFORE the import:
  scipy.misc.factorial   -> scipy.special.factorial (it takes vol.py's float32 argument; exact=False, as the old default)
  scipy.inf              -> numpy.inf
Nothing else is touched: cmdet, pdist, l2_distance and update_w run as written.

dist.py:73-82 (cosine_distance) cannot run on dense data with more than one sample (gen_golden_sivm.py); for the cosine-start
golden the reference runs with that one function replaced by the formula it states for a single vector, and the file says so
(cosine_patched).  Only SIVM's start uses it: the volumes are l2 whatever dist_measure says.
Only inputs and outputs are stored.  The reference is fed float64 arrays holding float32-representable values."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden_cnmf import seeded  # noqa: E402
from gen_golden_sivm import cosine_single, load_sivm  # noqa: E402
import sgreedy_cases as gc  # noqa: E402


def load_sgreedy():
    import scipy
    import scipy.special
    misc = types.ModuleType("scipy.misc")
    misc.factorial = scipy.special.factorial
    sys.modules["scipy.misc"] = misc
    scipy.misc = misc
    if not hasattr(scipy, "inf"):
        scipy.inf = np.inf
    load_sivm()
    return importlib.import_module("pymf.sivm_sgreedy")


def main():
    mod = load_sgreedy()
    cases = {}

    def add(name, V, desc, k, metric="l2", init="fastmap", W=None):
        mdl = mod.SIVM_SGREEDY(V.astype(np.float64), num_bases=k, dist_measure=metric, init=init)
        patched = False
        if metric == "cosine":
            try:
                mdl._distance(0)
            except ValueError:                   # dist.py:80 broadcasts to n x n
                mdl._distfunc = cosine_single
                patched = True
        if W is not None:
            mdl.W = W.copy()
        mdl.factorize(compute_w=W is None)
        d = dict(desc)
        d.update(k=np.int64(k), metric=np.str_(metric), init=np.str_(init), W=np.asarray(mdl.W, dtype=np.float64),
                 H=np.asarray(mdl.H, dtype=np.float64), ferr=np.asarray(mdl.ferr, dtype=np.float64),
                 H_is_data_flow_pin=np.bool_(True), cosine_patched=np.bool_(patched))
        if W is None:
            d["select"] = np.asarray(mdl.select, dtype=np.int64)
            d["v"] = np.asarray(mdl._v, dtype=np.float64)
        cases[name] = d

    Vd = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]], dtype=np.float32)                      # sivm_sgreedy.py:76-80
    add("sgreedy_doc_2x3_k2", Vd, dict(V=Vd), 2)
    Vu = np.array([[1.5, 1.3], [1.2, 0.3]], dtype=np.float32)                                # sivm_sgreedy.py:86-91
    add("sgreedy_doc_userw", Vu, dict(V=Vu), 2, W=np.array([[1.0, 0.0], [0.0, 1.0]]))
    V, d = seeded(37, 29, 1, 0.0)
    add("sgreedy_37x29_k5", V, d, 5)
    for what in ("l2", "l1", "cosine", "origin"):
        name = "sgreedy_29x300_k6_" + what
        m, n, k, seed, metric, init, special = gc.CASES[name]
        add(name, gc.data(m, n, k, seed, special)[0], dict(case=np.str_(name)), k, metric=metric, init=init)

    for name, d in cases.items():
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
        print("%-28s select %s ferr %.6g%s" % (name, d.get("select"), float(d["ferr"][0]), "  (cosine patched)" if d["cosine_patched"] else ""))


if __name__ == "__main__":
    main()
