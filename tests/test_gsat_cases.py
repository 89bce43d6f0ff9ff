"""The inputs of the SIVM_GSAT device tests, without a GPU: the float64 twin (tests/gsat_oracle.py) reproduces every reference
golden, every decision has a margin that a float64 implementation with another summation order cannot flip, and the walks
swap often enough -- twice inside one batch at least once -- to exercise the relaunch behind an accepted probe."""
import numpy as np
import pytest

import gsat_cases as gc
import gsat_oracle as go
from conftest import load_golden


@pytest.mark.parametrize("name", gc.GOLDEN_CASES)
def test_twin_reproduces_the_golden(name):
    g = load_golden(name)
    assert np.array_equal(g["idx"], gc.draws(name))
    t = gc.twin(name, reference_f1=True)
    exact = gc.twin(name)
    assert np.array_equal(exact["slots"], g["slots"]) and exact["select"] == t["select"]
    assert max(abs(a - b) / b for a, b in zip(exact["v"], g["v"])) <= gc.GOLDEN_V_TOL
    assert np.array_equal(t["slots"], g["slots"])
    assert t["select"] == [int(s) for s in g["select"]]
    assert np.array_equal(t["W"], g["W"])
    assert len(t["v"]) == len(g["v"])
    dv = max(abs(a - b) / b for a, b in zip(t["v"], g["v"]))
    print("%s twin _v deviation %.3e, margin twin %.3e golden %.3e" % (name, dv, t["margin"], float(g["margin"])))
    assert dv <= 1e-12 and abs(t["V"] - float(g["vol"])) <= 1e-12 * float(g["vol"])
    assert abs(t["margin"] - float(g["margin"])) <= 1e-6 * float(g["margin"])


@pytest.mark.parametrize("name", gc.GOLDEN_CASES)
def test_golden_margins_and_swaps(name):
    g = load_golden(name)
    assert float(g["margin"]) >= gc.MIN_MARGIN
    assert int((g["slots"] >= 0).sum()) >= gc.MIN_SWAPS
    assert int((g["slots"] == -2).sum()) > 0                   # the `n not in select` branch is taken


@pytest.mark.parametrize("name", gc.TWIN_CASES)
def test_twin_case_margins_and_swaps(name):
    t = gc.twin(name)
    print("%s swaps %s margin %.3e" % (name, gc.swaps_per_batch(t["slots"]), t["margin"]))
    assert t["margin"] >= gc.MIN_MARGIN
    assert int((t["slots"] >= 0).sum()) >= gc.MIN_SWAPS


def test_two_swaps_inside_one_batch_and_a_partial_last_batch():
    per_batch = {name: gc.swaps_per_batch(load_golden(name)["slots"]) for name in gc.GOLDEN_CASES}
    assert any(max(p) >= 2 for p in per_batch.values())
    assert gc.spec("gsat_37x29_k5")["n"] < gc.BATCH
    s = gc.spec("gsat_29x300_k6_l2")
    assert s["niter"] > 2 * gc.BATCH and s["niter"] % gc.BATCH != 0
    g = load_golden("gsat_29x300_k6_l2")
    assert gc.launches(g["slots"]) > len(per_batch["gsat_29x300_k6_l2"])   # some batch is relaunched behind a swap


def test_reference_volumes_vanish_from_20_bases_on():
    """vol.py:30-31 with its float32 j: the denominator is a float32, inf from 20 bases on, so f1 = 0 (gsat_cases.py)"""
    for k, zero in ((2, False), (19, False), (20, True), (36, True), (64, True)):
        assert (go.f1(k - 1, reference=True) == 0.0) == zero, k
        assert go.f1(k - 1) != 0.0
    for k in range(2, 20):
        assert abs(go.f1(k - 1, reference=True) / go.f1(k - 1) - 1.0) <= 2.0 * gc.GOLDEN_V_TOL
    assert all(gc.spec(n)["k"] > gc.REFERENCE_MAX_K for n in gc.TWIN_CASES)


def test_degenerate_case_is_degenerate():
    s = gc.spec("gsat_16x120_k20")
    assert s["m"] + 1 < s["k"]


def test_draws_are_the_legacy_stream():
    np.random.seed(7)
    one_by_one = [int(np.floor(np.random.random() * 300)) for _ in range(50)]
    assert go.draws(7, 50, 300).tolist() == one_by_one
