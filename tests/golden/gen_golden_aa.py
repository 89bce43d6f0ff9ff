#!/usr/bin/env python3
"""Generate the AA golden vectors (tests/golden/aa_*.npz) by running the REAL reference pymf/aa.py, imported unmodified through
the shim of gen_golden.py.

Both half steps go through `cvxopt.solvers.qp`, which is not installed where the goldens are made: a stand-in module takes its
place whose `solvers.qp(P, q, G, h, A, b)` returns an EXACT minimiser of the problem the reference poses (x >= 0, sum x = 1).
The H step's Hessian W^T W is positive definite (tests/sivm_oracle.py: simplex_qp, as for the SIVM goldens).  The W step's
Hessian data^T data is n x n and singular as soon as n > m, so that solver cannot be used there: the stand-in factors
P = F^T F through its eigen-decomposition, recovers the point w with F^T w = -q and projects it onto the hull of the columns
of F (tests/aa_oracle.py: hull_qp).  The goldens therefore pin aa.py's DATA FLOW -- pinv, HB and FB with their signs and
float64 casts, the per-base scatter into beta, W = (beta data^T)^T, the loop of NMF.factorize -- NOT cvxopt's interior-point
digits.  Where n > m, beta is one of many minimisers: only W, H and ferr are meaningful there.
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
import aa_cases as ac  # noqa: E402
import aa_oracle as ao  # noqa: E402
import sivm_oracle as so  # noqa: E402


def exact_simplex_qp(P, q):
    P = np.asarray(P, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    s, U = np.linalg.eigh(0.5 * (P + P.T))
    if s[0] > 1e-10 * s[-1]:
        return so.simplex_qp(P, -q)
    keep = s > 1e-12 * s[-1]
    F = np.sqrt(s[keep])[:, None] * U[:, keep].T               # P = F^T F
    w = (U[:, keep].T.dot(-q)) / np.sqrt(s[keep])              # F^T w = -q on the range of P
    return ao.hull_qp(F, w)


def load_aa():
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
        k = np.asarray(P).shape[0]
        assert np.array_equal(np.asarray(G), -np.eye(k)) and not np.any(np.asarray(h)), "x >= 0 (aa.py:106-107,127-128)"
        assert np.array_equal(np.asarray(A), np.ones((1, k))) and np.array_equal(np.asarray(b), np.ones((1, 1))), "sum x = 1"
        return {"x": matrix(exact_simplex_qp(P, q)), "status": "optimal"}

    cv = types.ModuleType("cvxopt")
    cv.base = types.ModuleType("cvxopt.base")
    cv.base.matrix = matrix
    cv.solvers = types.ModuleType("cvxopt.solvers")
    cv.solvers.qp = qp
    cv.solvers.options = {}
    sys.modules.update({"cvxopt": cv, "cvxopt.base": cv.base, "cvxopt.solvers": cv.solvers})
    return importlib.import_module("pymf.aa")


def main():
    aa = load_aa()
    cases = {}

    def add(name, V, desc, k, niter, W0=None, H0=None, compute_w=True, seed=None):
        if seed is not None:
            np.random.seed(seed)
        mdl = aa.AA(V.astype(np.float64), num_bases=k)
        if W0 is not None:
            mdl.W = W0.copy()
        if H0 is not None:
            mdl.H = H0.copy()
            mdl.beta = np.zeros((k, V.shape[1]))
        mdl.factorize(niter=niter, compute_w=compute_w)
        d = dict(desc)
        d.update(k=np.int64(k), niter=np.int64(niter), W=np.asarray(mdl.W, dtype=np.float64), H=np.asarray(mdl.H, dtype=np.float64),
                 ferr=np.asarray(mdl.ferr, dtype=np.float64), is_data_flow_pin=np.bool_(True), compute_w=np.bool_(compute_w))
        if compute_w:
            d["beta"] = np.asarray(mdl.beta, dtype=np.float64)
        if seed is not None:
            d["seed"] = np.int64(seed)
        cases[name] = d

    Vd = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]], dtype=np.float32)                     # aa.py:58-66
    add("aa_doc_2x3_k2", Vd, dict(V=Vd), 2, 5, seed=7)
    Vu = np.array([[1.5], [1.2]], dtype=np.float32)                                          # aa.py:72-76
    add("aa_doc_userw", Vu, dict(V=Vu), 2, 5, W0=np.array([[1.0, 0.0], [0.0, 1.0]]), compute_w=False, seed=7)
    for name in ("37x29_k5", "29x300_k6"):
        V, k, H0, W0 = ac.data(name)
        add("aa_" + name, V, dict(case=np.str_(name)), k, 1, W0=W0, H0=H0)

    for name, d in cases.items():
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
        print("%-18s ferr %s" % (name, d["ferr"]))


if __name__ == "__main__":
    main()
