#!/usr/bin/env python3
"""Generate the sparse SIVM golden vectors (tests/golden/sivm_sparse_*.npz) by running the REAL reference pymf/sivm.py through the
shim of gen_golden_sivm.py (load_sivm; H through the exact stand-in for cvxopt described there):

  on toarray()            for 'l2', 'l1' and 'cosine' (cosine with dist.py's cosine_distance replaced as in gen_golden_sivm.py):
                          select, W, H -- the yardstick of the device classes on sparse data
  on the CSC matrix itself  for 'l2' (the only measure the reference's sparse branch can run, sivm.py:110-120, dist.py:37-42):
                          update_w alone (its update_h cannot take the sparse W); the file records whether the two selections
                          agree (csc_run_agrees); this script asserts that they do on GOLDEN_CASES and that they do
                          not on DENSE_RUN_ONLY, whose files carry the run on toarray() as the yardstick.

Each file holds the CSC arrays of the case (tests/sivm_sparse_cases.py), float32 values."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden_sivm import cosine_single, load_sivm  # noqa: E402
import sivm_sparse_cases as ssc  # noqa: E402


# The cases whose CSC run in the reference agrees with its run on toarray().  On 29x300_k6, 31x300_k6 and 64x4113_k8 it does not:
# the expansion form of dist.py:37-42 gives sqrt(<0) = NaN for a column measured against itself and np.argmax picks that column
# again ([4, 35, 172, 208, 208, 208] on 29x300_k6) -- the re-pick that the device classes do not reproduce.
GOLDEN_CASES = ("5x37_k3", "29x300_k6_empty")
# the cases whose H the device tests compare and whose CSC run re-picks: the run on toarray() ties the oracle to the reference,
# the CSC run's selection is recorded with csc_run_agrees = False
DENSE_RUN_ONLY = ("29x300_k6", "31x300_k6")
# every cosine distance to the empty column 0, the fastmap start, is 1: column 0 wins every argmax and W has no H
DEGENERATE = ("29x300_k6_empty", "cosine")


def main():
    sivm = load_sivm()
    for name, metric in [(n, m) for n in GOLDEN_CASES + DENSE_RUN_ONLY for m in ssc.METRICS if (n, m) != DEGENERATE]:
        csc, V64, _ = ssc.data(name)
        k = ssc.spec(name)[2]
        mdl = sivm.SIVM(V64.copy(), num_bases=k, dist_measure=metric)
        patched = False
        if metric == "cosine":
            try:
                mdl._distance(0)
            except ValueError:                   # dist.py:80 broadcasts to n x n
                mdl._distfunc = cosine_single
                patched = True
        mdl.factorize()
        d = dict(case=np.str_(name), metric=np.str_(metric), init=np.str_("fastmap"), k=np.int64(k), shape=np.array(csc.shape, dtype=np.int64),
                 indptr=csc.indptr.astype(np.int64), indices=csc.indices.astype(np.int32), data=csc.data.astype(np.float32),
                 select=np.asarray(mdl.select, dtype=np.int64), W=np.asarray(mdl.W, dtype=np.float64), H=np.asarray(mdl.H, dtype=np.float64),
                 H_is_data_flow_pin=np.bool_(True), cosine_patched=np.bool_(patched))
        if metric == "l2":
            smdl = sivm.SIVM(csc.astype(np.float64), num_bases=k, dist_measure=metric)
            smdl.update_w()
            d["select_csc"] = np.asarray(smdl.select, dtype=np.int64)
            d["csc_run_agrees"] = np.bool_(list(smdl.select) == list(mdl.select))
            assert bool(d["csc_run_agrees"]) == (name in GOLDEN_CASES), (smdl.select, mdl.select)
        out = "sivm_sparse_%s_%s" % (name, metric)
        np.savez_compressed(os.path.join(HERE, out + ".npz"), **d)
        print("%-32s select %s%s" % (out, d["select"], "  (cosine patched)" if patched else ""))


if __name__ == "__main__":
    main()
