#!/usr/bin/env python3
"""Generate the vq / pdist golden vectors (tests/golden/vq_exact.npz, tests/golden/vq_generic.npz) by running the REAL reference
pymf/dist.py, imported unmodified through the shim of gen_golden.py (xrange), on the cases of tests/vq_cases.py.

The reference is fed float64 arrays holding the cases' float32 values.  Recorded per case, both metrics:
  cols_<metric>   vq(V, Q): for every query the nearest data column           (the direction of pmf_vq_columns)
  asg_<metric>    vq(Q, V): for every data column the nearest query           (the direction of pmf_vq_assign)
  pd_<metric>     pdist(Q, V), nq x n float64 -- for the exact cases with n <= 65, nq <= 17 and m in (1, 4, 65), and the first
                  PD_ROWS query rows and PD_COLS columns of every generic case (the files stay well below 1 MiB)
Exact cases: every shape of vq_cases.exact_shapes() with n <= 257 (the deep shapes have no golden: their expectation is the
same integer arithmetic).  Keys are "<case name>/<field>"."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import load_reference  # noqa: E402
import vq_cases as vc  # noqa: E402

PD_ROWS, PD_COLS = 4, 1024


def wants_pdist(m, n, nq):
    return n <= 65 and nq <= 17 and m in (1, 4, 65)


def main():
    load_reference()
    dist = importlib.import_module("pymf.dist")
    exact, generic = {}, {}
    for m, n, nq in vc.exact_shapes():
        if n > 257:
            continue
        c = vc.exact(m, n, nq)
        V, Q = c.V.astype(np.float64), c.Q.astype(np.float64)
        for k in vc.METRICS:
            exact["%s/cols_%s" % (c.name, k)] = dist.vq(V, Q, metric=k).astype(np.int32)
            exact["%s/asg_%s" % (c.name, k)] = dist.vq(Q, V, metric=k).astype(np.int32)
            if wants_pdist(m, n, nq):
                exact["%s/pd_%s" % (c.name, k)] = dist.pdist(Q, V, metric=k)
    for name in vc.generic_specs():
        c = vc.generic(name)
        V, Q = c.V.astype(np.float64), c.Q.astype(np.float64)
        for k in vc.METRICS:
            generic["%s/cols_%s" % (name, k)] = dist.vq(V, Q, metric=k).astype(np.int32)
            generic["%s/asg_%s" % (name, k)] = dist.vq(Q, V, metric=k).astype(np.int32)
            generic["%s/pd_%s" % (name, k)] = dist.pdist(Q, V, metric=k)[:PD_ROWS, :PD_COLS]
    np.savez_compressed(os.path.join(HERE, "vq_exact.npz"), **exact)
    np.savez_compressed(os.path.join(HERE, "vq_generic.npz"), **generic)
    for f in ("vq_exact.npz", "vq_generic.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
