"""The SIVM_CUR cases leave room for the comparison on the device (no GPU): every argmax of both selections keeps its gap in
float64 and with float32 distances (the two ties by construction are held to what they are), the kept eigenvalues of C^T C and
R R^T are away from svd.py's 1e-8 cut on both sides, the shapes reach the paths they are there for, and the oracle-vs-twin
deviations are the figures the device tolerances are made of."""
import os
import re

import numpy as np
import pytest

import sivm_cases as sc
import sivm_cur_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(cc.CASES) + list(cc.GOLDEN_ONLY)


def test_constants_match_the_library():
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_sivm.h")) as f:
        dev = f.read()
    assert int(re.search(r"PMF_SIVM_SLAB = (\d+);", dev).group(1)) == cc.SLAB
    assert int(re.search(r"PMF_SIVM_ROWS_WAVE = (\d+);", dev).group(1)) * 4 == cc.ROWS_WG
    import pymf_amd.sivm_cur as m
    assert m.MAX_BASES == cc.MAX_BASES == 64 and m.MAX_SHORT_SIDE == 16384
    assert int(re.search(r"PMF_SIVM_ROW_MAX_C = (\d+);", dev).group(1)) == m.MAX_SHORT_SIDE


def test_shapes_cover_the_paths():
    shape = {n: cc.CASES[n][:3] for n in cc.CASES}
    assert shape["5x37"][0] % 4 and shape["5x37"][0] < 64 and shape["5x37"][1] < cc.SLAB
    rows, cols, rrank = shape["40x4133"]
    assert cols // cc.SLAB >= 2 and 0 < cols % cc.SLAB < cc.SLAB and cols % 4 and rrank == 8     # three slabs, the last quad ragged
    rows, cols, _ = shape["300x29"]
    assert rows // cc.ROWS_WG >= 2 and rows % cc.ROWS_WG and cols < 64
    rows, cols, _ = shape["130x2100"]
    assert rows > cc.ROWS_WG and rows % cc.ROWS_WG and cols > cc.SLAB
    assert shape["64x2048_r64"] == (64, 2048, cc.MAX_BASES)
    assert {cc.CASES[n][6] for n in cc.CASES if n.startswith("29x300") and cc.CASES[n][7] == "origin"} == {"l2", "l1", "cosine"}
    assert cc.CASES["29x300_fastmap"][6:] == ("l2", "fastmap") and cc.CASES["29x300_offset1000"][4] == 1000.0


def test_doc_case_selects_the_origin_only():
    c = cc.case("doc_2x3")
    assert c["rid"] == [-1] and c["cid"] == [-1]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_well_posed(name):
    c = cc.case(name)
    for side, sel, scores in (("rows", c["rid"], c["scores_r"]), ("cols", c["cid"], c["scores_c"])):
        print(name, side, sel, "gaps %s" % ["%.1e" % g[0] for g in cc.gaps(scores, sel, c["init"])])
    g = c["gram"]
    print("kept_c [%.3e, %.3e] kept_r [%.3e, %.3e] dropped %s %s" % (g["kept_c"].min(), g["kept_c"].max(), g["kept_r"].min(), g["kept_r"].max(),
                                                                  g["dropped_c"], g["dropped_r"]))
    assert cc.well_posed(name, c) is None
    assert all(type(s) is int for s in c["rid"] + c["cid"])
    if c["init"] == "origin":
        assert c["rid"][0] == -1 and c["cid"][0] == -1
    # a -1 entry that meets a later selection of the last row / column: the Gram matrix has a null eigenvalue, and it is dropped
    last_r, last_c = c["data"].shape[0] - 1, c["data"].shape[1] - 1
    assert len(g["dropped_r"]) == (1 if (-1 in c["rid"] and last_r in c["rid"]) else 0)
    assert len(g["dropped_c"]) == (1 if (-1 in c["cid"] and last_c in c["cid"]) else 0)


def test_a_case_meets_the_last_row_again():
    """64 rows of 64 under 'origin': -1 is row 63, and the 63 argmaxes behind it take 63 distinct rows, so either row 63 comes
    again (a null eigenvalue to drop) or exactly one other row is left out."""
    c = cc.case("64x2048_r64")
    assert len(set(c["rid"][1:])) == 63 and len(set(c["cid"])) == 64
    print("row 63 again:", 63 in c["rid"], "dropped_r", c["gram"]["dropped_r"])


def test_the_tie_case_is_a_tie():
    c = cc.case(cc.TIE_CASE)
    rows, cols, rrank, seed, offset, scale, metric, init = cc.CASES[cc.TIE_CASE]
    src, dup = cc.tie_rows(cc.spectrum_data(rows, cols, seed, offset, scale), rrank, metric, init)
    assert src < dup and np.array_equal(c["data"][src], c["data"][dup])
    assert c["rid"][cc.TIE_ROUND] == src and dup not in c["rid"]
    s = c["scores_r"][cc.TIE_ROUND - 1]
    assert s[src] == s[dup] == s.max() and int(np.argmax(s)) == src


def test_cosine_under_origin_starts_with_an_all_equal_round():
    c = cc.case("29x300_cosine")
    for sel, scores in ((c["rid"], c["scores_r"]), (c["cid"], c["scores_c"])):
        assert np.all(scores[0] == scores[0][0]) and sel[:2] == [-1, 0]


@pytest.mark.parametrize("name", NAMES)
def test_twin_deviations(name):
    c = cc.case(name)
    du, df = cc.u_deviation(c), cc.ferr_deviation(c)
    print("%s: U deviation %.3e, ferr deviation %.3e" % (name, du, df))
    assert du <= cc.TWIN_U_DEV * 1.001 and df <= cc.TWIN_FERR_DEV * 1.001
    assert np.array_equal(c["twin"]["C"], c["C"]) and np.array_equal(c["twin"]["R"], c["R"])


def test_the_figures_are_the_worst_measured():
    worst_u = max(cc.u_deviation(cc.case(n)) for n in cc.CASES)
    worst_f = max(cc.ferr_deviation(cc.case(n)) for n in cc.CASES)
    assert 0.5 * cc.TWIN_U_DEV <= worst_u <= cc.TWIN_U_DEV * 1.001        # (the eigensolver and the BLAS at hand move the last digits)
    assert worst_f <= cc.TWIN_FERR_DEV * 1.001
    assert sc.MIN_GAP == 1e-3
