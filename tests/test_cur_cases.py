"""The CUR / CMD cases leave room for the comparison on the device (no GPU): no draw sits close enough to a cumulative
probability for the summation order to change an index, the kept eigenvalues of C^T C and R R^T are far above svd.py's 1e-8
cut and the dropped ones far below, the Gram form of the middle factor is the reference's pinv(C) data pinv(R), and the
device tolerance of each case separates a float64 middle product from a float32 one."""
import os
import re

import numpy as np
import pytest

import cur_cases as cc
import cur_oracle as co
import svd_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(name, kind) for name in sorted(cc.CUR_CASES) for kind in cc.KINDS]


def test_constants_match_the_library():
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_cur.h")) as f:
        dev = f.read()
    assert int(re.search(r"PMF_CUR_MAX_RANK = (\d+);", dev).group(1)) == cc.MAX_RANK
    import pymf_amd.cur
    assert pymf_amd.cur.MAX_RANK == cc.MAX_RANK


def test_shapes_cover_the_paths():
    """The cross product and the Gram matrix are one kernel, k_prod_f64, and share svd_chunks: one chunk, four chunks with a ragged tail, two tiles per output side."""
    assert sc.chunks(320, 1) == (1, 320)                       # 29 x 300: T = V Rg^T, one tile, one chunk
    assert sc.chunks(2112, 1) == (4, 576)                      # 29 x 2100
    assert sc.chunks(2112, 3 * 2) == (4, 576)                  # 130 x 2100 with 70 rows: 3 x 2 tiles, the last chunk 384 long
    assert sc.chunks(2112, 2 * 3) == (4, 576)                  # 2100 x 130: T' = Cg^T V, inner dimension the rows
    for name in ("130x2100", "2100x130"):
        for kind in cc.KINDS:
            c = cc.case(name, kind)
            assert len(c["rid"]) > 64 or kind == "cmd"          # more than one 64-wide tile of sampled rows / columns
    cur = cc.case("130x2100", "cur")
    assert len(set(cur["rid"].tolist())) < len(cur["rid"])     # repeated rows: R R^T is singular for CUR ...
    assert cc.case("130x2100", "cmd")["rcnt"].max() > 1        # ... and CMD carries counts above 1
    assert len(cc.case("200x200", "cur")["rid"]) == cc.MAX_RANK


@pytest.mark.parametrize("name,kind", PAIRS)
def test_case_is_well_posed(name, kind):
    c = cc.case(name, kind)
    g = c["gram"]
    d64 = c["data"].astype(np.float64)
    # draw margin: the summation order of the norms cannot change an index
    print("%s %s draw margin %.3e" % (kind, name, min(c["margins"])))
    assert min(c["margins"]) >= 1e-9
    # spectrum
    kept = np.concatenate([g["kept_c"], g["kept_r"]])
    dropped = np.concatenate([g["dropped_c"], g["dropped_r"], [0.0]])
    print("kept [%.3e, %.3e]  dropped <= %.3e  kappa_c %.3e  kappa_r %.3e" % (kept.min(), kept.max(), np.abs(dropped).max(),
                                                                              c["kappa_c"], c["kappa_r"]))
    assert kept.min() >= 1e-3 and np.abs(dropped).max() <= 1e-10 and kept.max() <= 1e6
    # formula: the twin's U (Gram form on the same float32-representable data) is the oracle's
    formula = cc.rel_max(c["twin"]["U"], c["U"])
    print("formula %.3e" % formula)
    assert formula <= 1e-9
    assert np.array_equal(c["twin"]["C"], c["C"]) and np.array_equal(c["twin"]["R"], c["R"])
    # tolerance: the device's bound on U tells float64 from float32
    u32 = co.gram_form(d64, c["rid"], c["rcnt"], c["cid"], c["ccnt"], middle32=True)["U"]
    effect = cc.rel_max(u32, c["U"])
    print("tol_U %.3e  float32 middle product %.3e  (%.1f x)" % (c["tol_U"], effect, effect / c["tol_U"]))
    if name == "doc_2x3":
        # cur.py's own example holds small integers: its float32 products are exact, there is nothing to tell apart
        assert effect <= 1e-15
    else:
        assert c["tol_U"] <= 0.1 * effect


def test_committed_tolerances_are_the_measured_ones():
    tol = cc.tolerances()
    got = cc.measure()
    assert sorted(tol["cases"]) == sorted(got)
    for key, fig in got.items():
        for q, v in fig.items():
            t = tol["cases"][key][q]
            if q == "ferr":                                    # (the float32 product of the twin follows the BLAS at hand)
                assert v <= tol["ferr_max"], (key, q, v)
            else:
                assert 0.9 * t <= v <= t * (1 + 1e-6), (key, q, v, t)    # (rounded up to two digits)
    assert tol["ferr_max"] == max(f["ferr"] for f in tol["cases"].values())
