"""The CURSL cases leave room for the comparison on the device (no GPU): the gap at the cut bounds what the eigen-solver's
error can do to the cumulative probabilities (tol_cum), no draw sits within 100 tol_cum of a cumulative probability, the kept
eigenvalues of the data's Gram matrix and of the sampled C^T C and R R^T are far above svd.py's 1e-8 cut and the dropped
ones far below."""
import os
import re

import numpy as np
import pytest

import cur_cases as cc
import cursl_cases as csc
import cursl_oracle as cso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(csc.CURSL_CASES)


def test_constants_match_the_library():
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_lev.h")) as f:
        dev = f.read()
    assert int(re.search(r"PMF_LEV_MAX_K = (\d+);", dev).group(1)) == csc.MAX_K
    assert int(re.search(r"PMF_LEV_PANEL = (\d+);", dev).group(1)) == 256
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_svd.h")) as f:
        svd = f.read()
    import pymf_amd.cursl
    assert int(re.search(r"PMF_SVD_MAX_RANK = (\d+);", svd).group(1)) == pymf_amd.cursl.MAX_SHORT_SIDE


def test_shapes_cover_the_paths():
    def tiles(name):
        c = csc.case(name)
        rows, cols = c["data"].shape
        kk_long = c["kk_r"] if rows > cols else c["kk_c"]
        return (kk_long + 15) // 16, -(-min(rows, cols) // 64), -(-max(rows, cols) // 64)
    # (operand tiles, pieces of the inner dimension, 64-wide panels of the long side)
    assert tiles("37x29") == (1, 1, 1) and csc.case("37x29")["kk_r"] == 5
    assert tiles("29x300") == (1, 1, 5)                        # two workgroups, the second with one active wave
    assert tiles("29x300_full") == (2, 1, 5) and csc.case("29x300_full")["kk_c"] == 29
    assert tiles("29x2100") == (2, 1, 33)                      # 33 = 8 x 4 + 1: a last workgroup with one active wave
    assert tiles("130x2100") == (5, 3, 33) and tiles("2100x130") == (5, 3, 33)
    assert tiles("200x200") == (8, 4, 4) and csc.case("200x200")["kk_c"] == csc.MAX_K
    assert tiles("300x2432") == (1, 5, 38)
    assert csc.case("29x300_full")["gram"]["dropped_c"].size > 0            # repeated columns of rank-29 data
    assert csc.case("130x2100")["rcnt"].max() > 1 or csc.case("130x2100")["ccnt"].max() > 1


@pytest.mark.parametrize("name", NAMES)
def test_case_is_well_posed(name):
    c = csc.case(name)
    # the gap at the cut
    lam, rank = c["lam"], int(np.sum(c["lam"] > cso.EPS))
    g = max(cso.gap_factor(lam, min(k, rank)) for k in (c["k_rows"], c["k_cols"]))
    assert c["g"] == g and c["tol_cum"] == cc.JACOBI_RTOL * g
    assert c["kk_r"] == min(c["k_rows"], rank) and c["kk_c"] == min(c["k_cols"], rank)
    assert abs(c["lev_r"].sum() - c["kk_r"]) <= 1e-12 * c["kk_r"] and abs(c["lev_c"].sum() - c["kk_c"]) <= 1e-12 * c["kk_c"]
    # draw margin
    print("%s g %.3f tol_cum %.3e draw margin %.3e (%.0f x)" % (name, g, c["tol_cum"], min(c["margins"]), min(c["margins"]) / c["tol_cum"]))
    assert min(c["margins"]) >= csc.MARGIN_FACTOR * c["tol_cum"]
    # the data's own spectrum
    kept, dropped = lam[lam > cso.EPS], lam[lam <= cso.EPS]
    assert kept.min() >= 1e-3 and np.abs(dropped).max(initial=0.0) <= 1e-10
    # the sampled Gram matrices
    gr = c["gram"]
    kept = np.concatenate([gr["kept_c"], gr["kept_r"]])
    dropped = np.concatenate([gr["dropped_c"], gr["dropped_r"], [0.0]])
    print("kept [%.3e, %.3e]  dropped <= %.3e  kappa_c %.3e  kappa_r %.3e" % (kept.min(), kept.max(), np.abs(dropped).max(),
                                                                              c["kappa_c"], c["kappa_r"]))
    assert kept.min() >= 1e-3 and np.abs(dropped).max() <= 1e-10
    assert max(c["kappa_c"], c["kappa_r"]) <= 1e4
    assert cc.rel_max(c["twin"]["U"], c["U"]) <= 1e-9


def test_committed_tolerances_are_the_measured_ones():
    tol = csc.tolerances()
    got = csc.measure()
    assert sorted(tol["cases"]) == sorted(got)
    for key, fig in got.items():
        for q, v in fig.items():
            t = tol["cases"][key][q]
            if q == "ferr":                                    # (the float32 product of the twin follows the BLAS at hand)
                assert v <= tol["ferr_max"], (key, q, v)
            else:
                assert 0.9 * t <= v <= t * (1 + 1e-6), (key, q, v, t)    # (rounded up to two digits)
    assert tol["ferr_max"] == max(f["ferr"] for f in tol["cases"].values())
