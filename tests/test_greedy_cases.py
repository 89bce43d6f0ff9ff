"""What makes the device comparison of tests/test_gpu_greedy.py meaningful, without a GPU: every round of every case keeps the
argmax gap, the float32 twin selects as the oracle does, and its deviations of H and ferr are the figures in greedy_cases.py."""
import numpy as np
import pytest

import greedy_cases as gc
import greedy_oracle as go


@pytest.mark.parametrize("name", list(gc.GREEDY_CASES))
def test_every_round_keeps_the_gap(name):
    c = gc.case(name)
    print(name, min(c["gaps"]))
    assert len(c["gaps"]) == c["num_bases"] and min(c["gaps"]) >= gc.MIN_GAP
    assert len(set(c["select"])) == c["num_bases"]


@pytest.mark.parametrize("name", gc.h_cases() )
def test_twin_selects_alike_and_deviations_are_the_committed_figures(name):
    c = gc.case(name)
    assert c["twin"]["select"] == c["select"]
    dh, df = gc.rel_max(c["twin"]["H"], c["H"]), gc.ferr_deviation(c)
    print(name, dh, df)
    assert dh <= gc.TWIN_H_DEV and df <= gc.TWIN_FERR_DEV


def test_the_figures_are_attained():
    assert gc.rel_max(gc.case("300x29_k6")["twin"]["H"], gc.case("300x29_k6")["H"]) >= 0.95 * gc.TWIN_H_DEV
    assert gc.ferr_deviation(gc.case("29x300_k6")) >= 0.95 * gc.TWIN_FERR_DEV
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
