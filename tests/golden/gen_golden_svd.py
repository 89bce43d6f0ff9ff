#!/usr/bin/env python3
"""Generate the SVD / PCA golden vectors (tests/golden/svd_*.npz, pca_*.npz) by running the REAL reference pymf/svd.py and
pymf/pca.py, imported unmodified through the shim of gen_golden.py, on the cases of tests/svd_cases.py, and write the
oracle-vs-twin figures of those cases to tests/golden/svd_tolerances.json (rounded up to two digits; tests/test_svd_cases.py
re-measures them and holds them to the file).

The reference is fed float64 arrays holding float32-representable values.  The two-tile shapes would not fit the size of a
committed golden with all of U, S, V: their goldens keep S, the rank, ferr and the leading 8 singular pairs."""
import importlib
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import load_reference  # noqa: E402
import svd_cases as sc  # noqa: E402

LEAD = 8                 # singular pairs kept in the goldens of the large cases
LARGE = 32 * 1024        # elements of U and V together beyond which only the leading pairs are kept


def round_up_2(x):
    if x <= 0.0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return math.ceil(x / 10.0 ** e) * 10.0 ** e


def main():
    load_reference()
    svd = importlib.import_module("pymf.svd")
    pca = importlib.import_module("pymf.pca")
    for name in sc.SVD_CASES:
        data = sc.svd_data(name)
        mdl = svd.SVD(data.astype(np.float64))
        mdl.factorize()
        U, S, V = np.asarray(mdl.U), np.asarray(mdl.S), np.asarray(mdl.V)
        d = dict(case=np.str_(name), rank=np.int64(S.shape[0]), S=np.diag(S).copy(), ferr=np.float64(mdl.frobenius_norm()))
        if U.size + V.size > LARGE:
            d.update(U=U[:, :LEAD], V=V[:LEAD], lead=np.int64(LEAD))
        else:
            d.update(U=U, V=V, lead=np.int64(S.shape[0]))
        np.savez_compressed(os.path.join(HERE, "svd_" + name + ".npz"), **d)
        print("svd_%-16s rank %3d ferr %.3e" % (name, d["rank"], d["ferr"]))
    for name in sc.PCA_CASES:
        data, nb, cm = sc.pca_data(name)
        mdl = pca.PCA(data.copy(), num_bases=nb, center_mean=cm)
        mdl.factorize()
        d = dict(case=np.str_(name), num_bases=np.int64(nb), center_mean=np.bool_(cm), W=np.asarray(mdl.W), H=np.asarray(mdl.H),
                 eigenvalues=np.asarray(mdl.eigenvalues), ferr=np.asarray(mdl.ferr, dtype=np.float64))
        np.savez_compressed(os.path.join(HERE, "pca_" + name + ".npz"), **d)
        print("pca_%-16s W %s ferr %.3e" % (name, d["W"].shape, d["ferr"][0]))
    # pca.py:57-66: coefficients for an existing basis
    Vu = np.array([[1.5], [1.2]])
    mdl = pca.PCA(Vu.copy(), num_bases=2)
    mdl.W = np.array([[1.0, 0.0], [0.0, 1.0]])
    mdl.factorize(compute_w=False)
    np.savez_compressed(os.path.join(HERE, "pca_doc_userw.npz"), data=Vu, W=np.asarray(mdl.W), H=np.asarray(mdl.H),
                        ferr=np.asarray(mdl.ferr, dtype=np.float64), cdata=np.asarray(mdl.data))
    measured = {q: round_up_2(v) for q, v in sc.measure().items()}
    with open(sc.TOL_PATH, "w") as f:
        json.dump({"what": "largest deviation of the float32 twin from the float64 oracle over the cases of tests/svd_cases.py "
                           "(svd_cases.svd_deviation / pca_deviation), rounded up to two digits; the device tolerances are "
                           "%g x these" % sc.FACTOR, "measured": measured}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(measured)


if __name__ == "__main__":
    main()
