#!/usr/bin/env python3
"""Generate the SIVM golden vectors (tests/golden/sivm_*.npz) by running the REAL reference pymf/sivm.py (with pymf/aa.py,
its base class), imported unmodified through the shim of gen_golden.py.

`select` and W involve no third-party code: they are true reference outputs.  H and ferr come out of aa.py:93-111 through
`cvxopt.solvers.qp`, which is not installed where the goldens are made (as for NMFALS, gen_golden.load_reference_nmfals): a
stand-in module takes its place whose `solvers.qp(P, q, G, h, A, b)` returns the EXACT minimiser of the problem the reference
poses (x >= 0, sum x = 1; tests/sivm_oracle.py: simplex_qp).  The H goldens therefore pin aa.py's data flow -- HA, FA with
their signs and float64 casts, the per-column scatter -- NOT cvxopt's interior-point digits.

dist.py:73-82 (cosine_distance) cannot run on dense data with more than one sample: tmp / k broadcasts an (n, 1) against an
(n,) array to n x n values, which sivm.py:133 cannot store.  For the cosine golden the reference runs with that one function
replaced by the formula it states for a single vector, 1 - d^T vec / (|d| |vec| + 1e-9); the file says so (cosine_patched).
The reference is fed float64 arrays holding float32-representable values."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import load_reference  # noqa: E402
from gen_golden_cnmf import seeded  # noqa: E402
import sivm_cases as sc  # noqa: E402
import sivm_oracle as so  # noqa: E402


def load_sivm():
    load_reference()

    class _Matrix(np.ndarray):
        pass

    def matrix(x, size=None):
        if size is not None:
            a = np.full(size, float(x), dtype=np.float64)
        else:
            a = np.array(x, dtype=np.float64)
            if a.ndim == 1:
                a = a.reshape(-1, 1)
        return a.view(_Matrix)

    def qp(P, q, G=None, h=None, A=None, b=None):
        P = np.asarray(P, dtype=np.float64)
        k = P.shape[0]
        assert np.array_equal(np.asarray(G), -np.eye(k)) and not np.any(np.asarray(h)), "x >= 0 (aa.py:106-107)"
        assert np.array_equal(np.asarray(A), np.ones((1, k))) and np.array_equal(np.asarray(b), np.ones((1, 1))), "sum x = 1 (aa.py:103,108)"
        return {"x": matrix(so.simplex_qp(P, -np.asarray(q, dtype=np.float64).reshape(-1))), "status": "optimal"}

    cv = types.ModuleType("cvxopt")
    cv.base = types.ModuleType("cvxopt.base")
    cv.base.matrix = matrix
    cv.solvers = types.ModuleType("cvxopt.solvers")
    cv.solvers.qp = qp
    cv.solvers.options = {}
    sys.modules.update({"cvxopt": cv, "cvxopt.base": cv.base, "cvxopt.solvers": cv.solvers})
    return importlib.import_module("pymf.sivm")


def cosine_single(d, vec):
    return 1.0 - np.dot(d.T, vec).reshape(-1) / (np.sqrt(np.sum(d ** 2, axis=0)) * np.sqrt(np.sum(vec ** 2)) + 10 ** -9)


def main():
    sivm = load_sivm()
    cases = {}

    def add(name, V, desc, k, metric="l2", init="fastmap", W=None):
        mdl = sivm.SIVM(V.astype(np.float64), num_bases=k, dist_measure=metric, init=init)
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
        cases[name] = d

    Vd = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]], dtype=np.float32)                      # sivm.py:58-61
    add("sivm_doc_2x3_k2", Vd, dict(V=Vd), 2)
    Vu = np.array([[1.5, 1.3], [1.2, 0.3]], dtype=np.float32)                                # sivm.py:67-71
    add("sivm_doc_userw", Vu, dict(V=Vu), 2, W=np.array([[1.0, 0.0], [0.0, 1.0]]))
    V, d = seeded(37, 29, 1, 0.0)
    add("sivm_37x29_k5", V, d, 5)
    for metric in ("l2", "l1", "cosine"):
        c = sc.CASES["29x300_k6_" + metric]
        V, _ = sc.planted(*c[:6], special=c[8])
        add("sivm_29x300_k6_" + metric, V, dict(case=np.str_("29x300_k6_" + metric)), 6, metric=metric)
    c = sc.CASES["29x300_k6_origin"]
    V, _ = sc.planted(*c[:6], special=c[8])
    add("sivm_29x300_k6_origin", V, dict(case=np.str_("29x300_k6_origin")), 6, init="origin")

    for name, d in cases.items():
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
        print("%-26s select %s ferr %.6g%s" % (name, d.get("select"), float(d["ferr"][0]), "  (cosine patched)" if d["cosine_patched"] else ""))


if __name__ == "__main__":
    main()
