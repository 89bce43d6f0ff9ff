#!/usr/bin/env python3
"""Generate the LAESA and GMAP golden vectors (tests/golden/laesa_*.npz, gmap_*.npz) by running the REAL reference
pymf/laesa.py and pymf/gmap.py (robust_map=False), imported unmodified through the shim of gen_golden.py.

As for SIVM (gen_golden_sivm.py): `select` and W are true reference outputs; H and ferr come out of aa.py:93-111 through the
stand-in for cvxopt that returns the exact minimiser, so the H goldens pin aa.py's data flow, not cvxopt's digits.  For LAESA
'cosine' the reference's cosine_distance, which cannot run on dense data with more than one sample, is replaced by the
formula it states for a single vector; the file says so (cosine_patched).  The reference is fed float64 arrays holding
float32-representable values; the 29 x 300 data are those of tests/colsel_cases.py."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden_cnmf import seeded  # noqa: E402
from gen_golden_sivm import cosine_single, load_sivm  # noqa: E402
import colsel_cases as cc  # noqa: E402


def main():
    load_sivm()
    laesa = importlib.import_module("pymf.laesa")
    sys.modules["dist"] = importlib.import_module("pymf.dist")     # kmeans.py:14, which gmap.py imports, says `import dist`
    gmap = importlib.import_module("pymf.gmap")
    cases = {}

    def add(name, make, V, desc, k, W=None, **meta):
        mdl = make(V.astype(np.float64))
        patched = False
        if meta.get("metric") == "cosine":
            try:
                mdl._distance(0)
            except ValueError:                   # dist.py:80 broadcasts to n x n
                mdl._distfunc = cosine_single
                patched = True
        if W is not None:
            mdl.W = W.copy()
        mdl.factorize(compute_w=W is None)
        d = dict(desc)
        d.update(k=np.int64(k), W=np.asarray(mdl.W, dtype=np.float64), H=np.asarray(mdl.H, dtype=np.float64),
                 ferr=np.asarray(mdl.ferr, dtype=np.float64), H_is_data_flow_pin=np.bool_(True), cosine_patched=np.bool_(patched))
        d.update({key: np.str_(v) for key, v in meta.items()})
        if W is None:
            d["select"] = np.asarray(mdl.select, dtype=np.int64)
        cases[name] = d

    def add_laesa(name, V, desc, k, metric="l2", init="fastmap", W=None):
        add(name, lambda D: laesa.LAESA(D, num_bases=k, dist_measure=metric, init=init), V, desc, k, W, metric=metric, init=init)

    def add_gmap(name, V, desc, k, method="pca", W=None):
        add(name, lambda D: gmap.GMAP(D, num_bases=k, method=method, robust_map=False), V, desc, k, W, method=method)

    Vd = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]], dtype=np.float32)                      # laesa.py:47-49, gmap.py:58-60
    Vu = np.array([[1.5, 1.3], [1.2, 0.3]], dtype=np.float32)                                # laesa.py:55-59, gmap.py:66-70
    Wu = np.array([[1.0, 0.0], [0.0, 1.0]])
    add_laesa("laesa_doc_2x3_k2", Vd, dict(V=Vd), 2)
    add_laesa("laesa_doc_userw", Vu, dict(V=Vu), 2, W=Wu)
    add_gmap("gmap_doc_2x3_k2", Vd, dict(V=Vd), 2)
    add_gmap("gmap_doc_userw", Vu, dict(V=Vu), 2, W=Wu)
    V, d = seeded(37, 29, 1, 0.0)
    add_gmap("gmap_37x29_k5", V, d, 5)
    for tail in ("l2", "l1", "cosine", "origin"):
        name = "laesa_29x300_k6_" + tail
        rule, m, n, k, seed, metric, init, special = cc.CASES[name]
        add_laesa(name, cc.data(rule, m, n, k, seed, metric, special)[0], dict(case=np.str_(name)), k, metric=metric, init=init)
    for method in ("pca", "aa", "nmf"):
        name = "gmap_29x300_k6_" + method
        rule, m, n, k, seed, _, _, special = cc.CASES[name]
        add_gmap(name, cc.data(rule, m, n, k, seed, method, special)[0], dict(case=np.str_(name)), k, method=method)

    for name, d in cases.items():
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
        print("%-26s select %s ferr %.6g%s" % (name, d.get("select"), float(d["ferr"][0]), "  (cosine patched)" if d["cosine_patched"] else ""))


if __name__ == "__main__":
    main()
