"""What makes the device comparison of tests/test_gpu_greedy.py meaningful, without a GPU: every round of every case keeps the
argmax gap, the float32 twin selects as the oracle does, and its deviations of H and ferr are the figures in greedy_cases.py."""
import os
import re

import numpy as np
import pytest

import greedy_cases as gc
import greedy_oracle as go

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pymf_amd", "csrc")


@pytest.mark.parametrize("name", list(gc.GREEDY_CASES) + list(gc.SELECT_CASES))
def test_every_round_keeps_the_gap(name):
    c = gc.case(name)
    print(name, min(c["gaps"]))
    assert len(c["gaps"]) == c["num_bases"] and min(c["gaps"]) >= gc.MIN_GAP
    assert len(set(c["select"])) == c["num_bases"]


def header_constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


def test_the_wide_and_panel_cases_reach_the_branches_they_are_meant_for():
    """greedy_launch_pass, greedy_select (pmf_host_greedy.h) and k_greedy_pass, k_greedy_gram (pmf_greedy.h) restated on the
    shapes of the cases, with the constants read from the headers: a change of one of them that takes a case off its branch
    fails here."""
    max_wgs = header_constant("pmf_cluster.h", "PMF_CL_MAX_WGS")
    mc = header_constant("pmf_greedy.h", "PMF_GREEDY_MC")
    opw = header_constant("pmf_greedy.h", "PMF_GREEDY_OPW")

    def tiles(name):                             # NT of every round: the operand holds c + i columns (c = num_bases: full rank)
        rows, cols, k, _ = gc.GREEDY_CASES.get(name) or gc.SELECT_CASES[name]
        assert k <= min(rows, cols) and k + k - 1 <= opw
        return [-(-(k + i) // 16) for i in range(k)]

    def pass_smem(nt):                           # greedy_pass_smem<NT>: PMF_GREEDY_MC rows of greedy_ldr<NT>() floats
        return mc * (16 * nt if (16 * nt) % 32 == 16 else 16 * nt + 16) * 4

    for name in ("80x640_k64", "80x2048_k64"):
        assert sorted(set(tiles(name))) == [4, 5, 6, 7, 8]
    assert max(max(tiles(n)) for n in gc.GREEDY_CASES if n != "80x640_k64") == 6        # nothing else reaches 7 and 8
    assert pass_smem(8) == 73728 > 65536 >= pass_smem(7)                                 # <8> alone raises its LDS limit
    assert -(-2048 // 64) == 32                  # 80x2048_k64: one panel per workgroup, one workgroup per panel

    def ranges(name):
        rows, cols, _, _ = gc.SELECT_CASES[name]
        panels = -(-cols // 64)
        ppw = -(-panels // min(panels, max_wgs))
        wgs = -(-panels // ppw)
        # panels, per workgroup, workgroups, panels of the last workgroup, columns of the last panel, trips of the panel loop
        # (four waves a trip) of a full workgroup, LDS row chunks
        return panels, ppw, wgs, panels - (wgs - 1) * ppw, cols - (panels - 1) * 64, -(-ppw // 4), -(-((rows + 3) // 4 * 4) // mc)

    assert ranges("8x65600_k3") == (1025, 2, 513, 1, 64, 1, 1)          # last workgroup: one panel, three idle waves
    assert ranges("8x262208_k2") == (4097, 5, 820, 2, 64, 2, 1)         # last workgroup: two panels, two idle waves
    assert ranges("132x262208_k2") == (4097, 5, 820, 2, 64, 2, 2)
    for name in gc.ROLL:                         # the rotated copies: the first winner in the fifth panel of its workgroup
        base = name[:-len("_roll")]
        assert ranges(name) == ranges(base) and gc.SELECT_CASES[name] == gc.SELECT_CASES[base]
        cols, ppw = gc.SELECT_CASES[name][1], ranges(name)[1]
        assert gc.case(name)["select"] == [(s + gc.ROLL[name]) % cols for s in gc.case(base)["select"]]
        assert [s // 64 % ppw for s in gc.case(base)["select"]][0] < 4 <= [s // 64 % ppw for s in gc.case(name)["select"]][0]
    # GREEDYCUR 300x130: more rows than columns, so the rows are chosen by the pass over the transposed copy -- k_greedy_transpose
    # on a grid of (rows / 64, cols / 64) padded tiles -- and the columns in Gram space
    rows, cols = gc.GREEDYCUR_CASES["300x130"][:2]
    assert rows > cols and (-(-rows // 64), -(-cols // 64)) == (5, 3)
    assert all(min(-(-r // 64), -(-c // 64)) == 1 for n, (r, c, _, _) in gc.GREEDYCUR_CASES.items() if n != "300x130" and r > c)
    # 1300x1100_k4: Gram space (rows > cols) with more candidates than k_greedy_gram has threads
    rows, cols = gc.SELECT_CASES["1300x1100_k4"][:2]
    assert rows > cols and 1024 < cols < 2048 and cols - 1024 == 76
    assert max(c for r, c, _, _ in gc.GREEDY_CASES.values() if r > c) <= 1024


@pytest.mark.parametrize("name", gc.h_cases() )
def test_twin_selects_alike_and_deviations_are_the_committed_figures(name):
    c = gc.case(name)
    assert c["twin"]["select"] == c["select"]
    dh, df = gc.rel_max(c["twin"]["H"], c["H"]), gc.ferr_deviation(c)
    print(name, dh, df)
    assert dh <= gc.TWIN_H_DEV and df <= gc.TWIN_FERR_DEV


def test_the_figures_are_attained():
    assert gc.rel_max(gc.case("300x29_k6")["twin"]["H"], gc.case("300x29_k6")["H"]) >= 0.95 * gc.TWIN_H_DEV
    assert gc.ferr_deviation(gc.case("80x640_k64")) >= 0.95 * gc.TWIN_FERR_DEV
    assert gc.ferr_deviation(gc.cur_case("40x300")) >= 0.95 * gc.TWIN_CUR_FERR_DEV


def test_planted_tie():
    c = gc.case(gc.TIE_CASE)
    src, dup = gc.tie_columns(gc.spectrum_data(64, 640, 8))
    assert dup > src and np.array_equal(c["data"][:, src], c["data"][:, dup])
    assert c["gaps"][0] == 0.0 and min(c["gaps"][1:]) >= gc.MIN_GAP      # an exact tie, then clear winners
    assert c["select"][0] == src and dup not in c["select"]


def test_rank_case():
    c = gc.case(gc.RANK_CASE)
    assert np.linalg.matrix_rank(c["data"].astype(np.float64), tol=1e-4) == gc.RANK
    assert min(c["gaps"][:gc.RANK - 1]) >= gc.MIN_GAP
    assert c["twin"]["select"][:gc.RANK - 1] == c["select"][:gc.RANK - 1]
    # the round that exhausts the rank: every column with a residual has the same score (see greedy_cases.py)
    T = c["scores"][gc.RANK - 1]
    tied = T >= T.max() * (1.0 - gc.TIE_RTOL)
    assert tied.sum() >= 290 and T[c["twin"]["select"][gc.RANK - 1]] >= T.max() * (1.0 - gc.TIE_RTOL)
    assert all(0 <= s < 300 for s in c["twin"]["select"]) and len(set(c["twin"]["select"])) == 5


@pytest.mark.parametrize("name", list(gc.GREEDYCUR_CASES))
def test_greedycur_cases(name):
    c = gc.cur_case(name)
    d = c["data"]
    assert min(c["gaps"]) >= gc.MIN_GAP
    assert go.select_twin(np.ascontiguousarray(d.T), c["rrank"]) == c["rid"] and go.select_twin(d, c["rrank"]) == c["cid"]
    assert gc.ferr_deviation(c) <= gc.TWIN_CUR_FERR_DEV
    assert 0.0 < c["tol_U"] < 1e-6


def test_replaced_data_keep_the_gap():
    gaps = []
    sel = go.select(gc.REPLACED_DATA().astype(np.float64), 6, gaps=gaps)
    assert min(gaps) >= gc.MIN_GAP and sel != gc.case("29x300_k6")["select"]
