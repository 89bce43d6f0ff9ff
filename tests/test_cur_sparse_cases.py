"""The sparse CUR / CMD cases leave room for the comparison on the device (no GPU): cur_cases' own well-posedness conditions
hold on toarray(), the data have the long and the empty lines that the kernels must get right, the trace identity of the
error is the direct error to rounding, and its cancellation stays out of the comparison."""
import numpy as np
import pytest

import cur_cases as cc
import cur_sparse_cases as scs

PAIRS = [(name, kind) for name in sorted(scs.SPARSE_CASES) for kind in scs.KINDS]


@pytest.mark.parametrize("name", sorted(scs.SPARSE_CASES))
def test_the_recipe_gives_long_and_empty_lines(name):
    m, n = scs.SPARSE_CASES[name][:2]
    A = scs.matrix(name)
    assert A.dtype == np.float32 and A.has_canonical_format and A.shape == (m, n)
    rows, cols = np.diff(A.indptr), np.diff(A.tocsc().indptr)
    assert rows[m // 3] == n - 2 and cols[n // 3] == m - 2        # full but for the two emptied crossings
    for r in (m // 2, m - 1):
        assert rows[r] == 0
    for c in (n // 2, 0):
        assert cols[c] == 0
    assert A.data.min() >= 0.25                                   # no stored zero changes a count above
    assert rows[m // 3] > 16 and cols[n // 3] > 16                # longer than a team of k_cur_csr_sqnorms
    # the same matrix again: the recipe is a function of the seed
    B = scs.matrix(name)
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


def test_shapes_cover_the_paths():
    cur = scs.case("130x2100", "cur")
    assert len(set(cur["rid"].tolist())) < len(cur["rid"])       # a repeated row: R R^T is singular for CUR ...
    assert scs.case("130x2100", "cmd")["rcnt"].max() > 1         # ... and CMD carries a count above 1
    assert len(scs.case("200x200", "cur")["rid"]) == cc.MAX_RANK
    assert len(scs.case("3000x2500", "cur")["rid"]) == 64 and len(scs.case("1100x4100", "cur")["rid"]) == 65
    for name in ("130x2100", "2100x130"):
        c = scs.case(name, "cur")
        assert len(c["rid"]) > 64 and len(c["cid"]) > 64          # two 64-wide tiles on either side
    # the full row is drawn where a selected row must span several 256-entry chunks of k_cur_csr_mid
    for name in ("130x2100", "3000x2500", "1100x4100"):
        m, n = scs.SPARSE_CASES[name][:2]
        assert m // 3 in scs.case(name, "cur")["rid"].tolist() and n - 2 > 256


@pytest.mark.parametrize("name,kind", PAIRS)
def test_case_is_well_posed(name, kind):
    c = scs.case(name, kind)
    g = c["gram"]
    print("%s %s draw margin %.3e" % (kind, name, min(c["margins"])))
    assert min(c["margins"]) >= 1e-9
    kept = np.concatenate([g["kept_c"], g["kept_r"]])
    dropped = np.concatenate([g["dropped_c"], g["dropped_r"], [0.0]])
    print("kept [%.3e, %.3e]  dropped <= %.3e  kappa_c %.3e  kappa_r %.3e" % (kept.min(), kept.max(), np.abs(dropped).max(),
                                                                              c["kappa_c"], c["kappa_r"]))
    assert kept.min() >= 1e-3 and np.abs(dropped).max() <= 1e-10 and kept.max() <= 1e6
    # the Gram form of the middle factor is the reference's pinv(C) data pinv(R)
    assert cc.rel_max(g["U"], c["U"]) <= 1e-9
    # the error is far from 0: the identity's cancellation stays out of the comparison
    print("ferr / ||data|| %.3f  identity vs direct %.3e" % (c["ferr"] / c["norm"], scs.twin_deviation(c)))
    assert c["ferr"] / c["norm"] >= scs.MIN_REL_FERR


def test_committed_tolerances_are_the_measured_ones():
    tol = scs.tolerances()
    got = scs.measure()
    assert sorted(tol["cases"]) == sorted(got)
    for key, fig in got.items():
        for q, v in fig.items():
            t = tol["cases"][key][q]
            if q == "ferr":                                    # (sums of 1e-16-sized roundings: they follow the BLAS at hand)
                assert cc.FACTOR * v <= scs.device_tol_ferr(), (key, q, v)
            elif q == "ferr_dense":                            # (the float32 product of the twin follows the BLAS at hand too)
                assert v <= tol["ferr_dense_max"], (key, q, v)
            else:
                assert 0.9 * t <= v <= t * (1 + 1e-6), (key, q, v, t)    # (rounded up to two digits)
    assert tol["ferr_max"] == max(f["ferr"] for f in tol["cases"].values())
    assert tol["ferr_dense_max"] == max(f["ferr_dense"] for f in tol["cases"].values())
    assert scs.device_tol_ferr() == max(cc.FACTOR * tol["ferr_max"], scs.FERR_FLOOR)
