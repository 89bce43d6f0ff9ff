"""pmf_chnmf_hull on the MI355X against exact integer geometry (tests/chnmf_exact_cases.py; what the cases are and why the
projection is exact: tests/test_chnmf_exact_cases.py, no GPU).  R and V hold small integers, so proj = R V is exact in any
summation order, every cross product of the filter and the chain is exact, and `_hull_idx` must be the strict hull computed
with Python integers -- through every route and partition, with no tolerance anywhere."""
import numpy as np
import pytest

import chnmf_exact_cases as ec
from pymf_amd import _lib

pytestmark = pytest.mark.gpu


def hull_twice(g, survivor_cap=0, max_wgs=0):
    """(_hull_idx, routes) of the case through the C ABI; a second call on the same context must give the same bytes (the mask,
    the counts and the survivor list are the context's and are reused)."""
    ctx = _lib.Context(_lib.ALGO_AA, g["m"], g["n"], min(2, g["n"]))
    try:
        ctx.set_v_dense(g["V"])
        ctx.chnmf_set_limits(survivor_cap, max_wgs)
        idx = ctx.chnmf_hull(g["R"])
        routes = ctx.chnmf_routes()
        again = ctx.chnmf_hull(g["R"])
        assert again.dtype == np.int32 and again.tobytes() == idx.tobytes(), (idx, again)
        assert ctx.chnmf_routes() == routes
    finally:
        ctx.close()
    return idx, routes


@pytest.mark.parametrize("name", list(ec.CASES))
def test_hull_is_the_exact_hull(name):
    g = ec.case(name)
    pairs = g["base_sel"] * (g["base_sel"] - 1) // 2
    for max_wgs in g["max_wgs"]:
        idx, routes = hull_twice(g, max_wgs=max_wgs)
        assert idx.dtype == np.int32
        assert np.array_equal(idx, g["hull"]), (max_wgs, idx, g["hull"])
        if g["routes"] == "device":                # n survivors <= the capacity in every pair, whatever the filter picks
            assert routes == (pairs, 0, 0)
        if g["routes"] == "host":                  # more than the capacity with either number of directions
            assert routes == (0, 0, pairs)


def test_survivors_equal_to_the_capacity():
    """survivor_cap = 64 and the 64 boundary points of the 17 x 17 grid: the chain's frame is exactly full."""
    g = ec.case("grid17")
    idx, _ = hull_twice(g, survivor_cap=ec.FORCED_CAP)
    assert idx.dtype == np.int32
    assert np.array_equal(idx, g["hull"]), (idx, g["hull"])


@pytest.mark.parametrize("name", ec.FORCED_CAP_CASES)
def test_rerun_and_host_routes_give_the_exact_hull(name):
    """survivor_cap = 64 with 72, 100 and 256 survivors: the 128-direction rerun runs, then the host forms the hull.  The first
    route is excluded by the geometry, not by the filter's picks: more than 64 points lie on the hull's boundary, and no polygon
    of data points has such a point strictly inside."""
    g = ec.case(name)
    idx, routes = hull_twice(g, survivor_cap=ec.FORCED_CAP)
    assert idx.dtype == np.int32
    assert np.array_equal(idx, g["hull"]), (idx, g["hull"])
    assert routes[0] == 0 and sum(routes) == g["base_sel"] * (g["base_sel"] - 1) // 2
