"""The exact-geometry CHNMF cases (tests/chnmf_exact_cases.py) are what they claim: the projection is exact in float64, every
cross product stays an exact integer, the Python-integer hull agrees with the NumPy restatement of both device stages
(tests/chnmf_cases.py), and every case reaches the edge it is in the table for.  No GPU."""
import numpy as np
import pytest

import chnmf_cases as cc
import chnmf_exact_cases as ec

NAMES = list(ec.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_projection_and_cross_products_are_exact(name):
    g = ec.case(name)
    assert g["V"].dtype == np.float32 and g["V"].shape == (g["m"], g["n"])
    assert g["R"].dtype == np.float64 and g["R"].shape == (g["base_sel"], g["m"])
    assert 2 <= g["base_sel"] <= min(16, g["m"]) and min(g["m"] + 1, g["n"]) <= 128        # what the AA context takes
    exact = g["R"].astype(np.int64).dot(g["V"].astype(np.int64))
    assert np.array_equal(exact, g["P"])
    P = cc.proj64(g["V"], g["R"])
    assert P.dtype == np.float64 and np.array_equal(P, exact.astype(np.float64)) and np.array_equal(P.astype(np.int64), exact)
    # every partial sum of an entry, in any order, is an integer of magnitude <= sum |R| |V|
    assert int(np.abs(g["R"].astype(np.int64)).dot(np.abs(g["V"].astype(np.int64))).max()) < ec.LIMIT
    assert int(np.abs(exact).max()) < ec.LIMIT
    # a cross product (a - o) x (b - o) and both of its products: |.| <= 2 (x range) (y range)
    rng = [int(r.max()) - int(r.min()) for r in exact]
    for i, j in cc.pairs(g["base_sel"]):
        assert 2 * rng[i] * rng[j] < ec.LIMIT


@pytest.mark.parametrize("name", NAMES)
def test_exact_hull_is_the_restated_chain_and_survives_both_filters(name):
    g = ec.case(name)
    hull = g["hull"]
    assert hull.dtype == np.int32 and np.all(np.diff(hull) > 0) and len(hull) >= 1
    P = cc.proj64(g["V"], g["R"])
    found = set()
    for i, j in cc.pairs(g["base_sel"]):
        want = ec.exact_hull(g["P"][i], g["P"][j])
        assert cc.chain_hull(P[i], P[j]) == want
        for D in (cc.D0, cc.D1):
            surv = cc.filter_survivors(P[i], P[j], D)
            assert cc.chain_hull(P[i][surv], P[j][surv], surv) == want
        found.update(want)
    assert np.array_equal(np.array(sorted(found), dtype=np.int32), hull)
    assert np.array_equal(cc.hull_union(g["V"], g["R"]), hull)


def test_exact_hull_by_hand():
    assert ec.exact_hull([5], [5]) == [0]
    assert ec.exact_hull([5, 5, 5], [5, 5, 5]) == [0]
    assert ec.exact_hull([1, 0, 0, 1], [1, 0, 0, 1]) == [1, 0]                       # two points, each twice
    assert ec.exact_hull([0, 1, 2], [0, 1, 2]) == [0, 2]                             # collinear
    assert ec.exact_hull([0, 2, 2, 0, 1, 1, 2], [0, 0, 2, 2, 0, 1, 1]) == [0, 1, 2, 3]   # edge and interior points are no vertices
    assert ec.exact_hull([2, 0, 0, 2, 0], [2, 0, 2, 0, 0]) == [1, 3, 0, 2]           # the duplicate of (0, 0) at column 4 is not named
    big = 2 ** 40
    assert ec.exact_hull([0, big, 2 * big, big], [0, big, 2 * big, big - 1]) == [0, 3, 2]     # 2^80 products: Python ints


def _survivors(g, i, j, D):
    P = g["P"].astype(np.float64)
    return cc.filter_survivors(P[i], P[j], D)


def test_what_the_cases_are_for():
    case = ec.case
    assert ec.CAP == cc.CAP
    # degenerate sets
    for name in ("identical_n1", "identical_n2", "identical_n64", "identical_n300"):
        assert list(case(name)["hull"]) == [0] and len(np.unique(case(name)["P"], axis=1).T) == 1
    assert [case(n)["n"] for n in ("identical_n1", "identical_n2", "identical_n64", "identical_n300")] == [1, 2, 64, 300]
    two = case("two_points_n12")
    assert len(np.unique(two["P"], axis=1).T) == 2 and list(two["hull"]) == [0, 1] and two["n"] == 12
    for name, fixed in (("line_horizontal", 1), ("line_vertical", 0), ("line_slope_3_7", None)):
        g = case(name)
        x, y = g["P"]
        if fixed is not None:
            assert len(set(g["P"][fixed].tolist())) == 1
        else:
            assert np.all(7 * (y - y[0]) == 3 * (x - x[0])) and len(set(x.tolist())) == g["n"] - 4
        assert len(g["hull"]) == 2
        for v in g["hull"]:                          # each endpoint three times; the vertex is the lowest index, and the copies
            same = np.nonzero((x == x[v]) & (y == y[v]))[0]          # do not follow it directly
            assert len(same) == 3 and same[0] == v and same[1] > v + 1
        assert len(_survivors(g, 0, 1, cc.D0)) == g["n"]             # nothing on a line is inside anything
    assert list(case("three_collinear")["hull"]) == [1, 2]
    # equal-x runs and lattice ties
    for name, w, copies in (("grid17", 17, 1), ("grid17_dup_corners", 17, 3), ("grid65", 65, 1)):
        g = case(name)
        x, y = g["P"]
        assert g["n"] == w * w + 4 * (copies - 1) and len(g["hull"]) == 4
        assert sorted(np.bincount(x - x.min()).tolist())[0] >= w     # every x is an equal-x run of at least w points
        for v in g["hull"]:
            same = np.nonzero((x == x[v]) & (y == y[v]))[0]
            assert abs(x[v]) == w // 2 and abs(y[v]) == w // 2 and len(same) == copies and same[0] == v
        on_boundary = int(((np.abs(x) == w // 2) | (np.abs(y) == w // 2)).sum())
        assert on_boundary == 4 * (w - 1) + 4 * (copies - 1)
        for D in (cc.D0, cc.D1):                                     # exactly the boundary survives: 15 (63) points on every edge
            assert len(_survivors(g, 0, 1, D)) == on_boundary
    assert len(_survivors(case("grid17"), 0, 1, cc.D0)) == ec.FORCED_CAP          # cnt == cap under the forced capacity
    assert case("grid65")["n"] > ec.CAP
    circ = case("circle65")
    x, y = circ["P"]
    on_circle = set(np.nonzero(x * x + y * y == 65 * 65)[0].tolist())
    assert len(on_circle) == 36 and on_circle <= set(circ["hull"].tolist()) and circ["n"] == 13273
    # duplicate runs across boundaries
    dup = case("dup_boundaries")
    assert dup["n"] == 5000 and dup["max_wgs"] == (1, 3, 0) and dup["base_sel"] == 3
    assert [ec.DUP_COLUMNS[k][:2] for k in "ABCD"] == [(63, 64), (255, 256), (1727, 1728), (4991, 4999)]
    assert 1728 == 27 * 64 and 4991 == 78 * 64 - 1 and 4999 == dup["n"] - 1
    for cols in ec.DUP_COLUMNS.values():
        assert len(np.unique(dup["P"][:, list(cols)], axis=1).T) == 1
        same = np.nonzero((dup["P"] == dup["P"][:, cols[0]:cols[0] + 1]).all(axis=0))[0]
        assert tuple(same) == cols                                   # no copy below the first of the pair
    assert list(dup["hull"]) == [cols[0] for cols in (ec.DUP_COLUMNS[k] for k in "ABCD")]
    x, y = dup["P"][:2]
    assert ((y == 0) & (x > 0) & (x < ec.DUP_SIDE)).sum() > 10 and ((x == ec.DUP_SIDE) & (y > 0) & (y < ec.DUP_SIDE)).sum() > 10
    # chain sizes: the survivor count is n, with either number of directions, in all three pairs
    sizes = {"parabola_1025": 1025, "parabola_2048": 2048, "parabola_2049": 2049, "parabola_4096": 4096, "parabola_4097": 4097}
    for name, n in sizes.items():
        g = case(name)
        assert g["n"] == n and g["base_sel"] == 3 and g["routes"] == ("device" if n <= ec.CAP else "host")
        assert len(g["hull"]) == n and int(g["P"][1].max()) == (n - 1) ** 2
        for i, j in cc.pairs(3):
            for D in (cc.D0, cc.D1):
                assert len(_survivors(g, i, j, D)) == n
        assert len(ec.exact_hull(g["P"][0], g["P"][1])) == n and len(ec.exact_hull(g["P"][0], g["P"][2])) == n
        assert len(ec.exact_hull(g["P"][1], g["P"][2])) == 2
    assert sizes["parabola_4096"] == ec.CAP and sizes["parabola_4097"] == ec.CAP + 1 and 4096 ** 2 == 2 ** 24
    over = case("over_cap_vertex")
    x, y = over["P"]
    assert len(over["hull"]) == 3 and over["routes"] == "host"
    runs = [np.nonzero((x == x[v]) & (y == y[v]))[0] for v in over["hull"]]
    assert sorted(len(r) for r in runs) == [1, 1, 4200] and all(r[0] == v for r, v in zip(runs, over["hull"]))
    assert max(runs, key=len)[0] > 0                                 # the run does not begin at column 0
    for D in (cc.D0, cc.D1):
        assert len(_survivors(over, 0, 1, D)) > ec.CAP
    # projection shapes
    ms = [case("proj_m%d" % m)["m"] for m in ec.PROJ_M]
    assert ms == ec.PROJ_M and set(m % 4 for m in ms) == {0, 1, 2, 3}
    assert all(case("proj_m%d" % m)["n"] == (320 if m <= 127 else 100) for m in ec.PROJ_M)
    assert all(case("proj_m%d" % m)["base_sel"] == min(4, m) for m in ec.PROJ_M)
    assert [case("proj_n%d" % n)["n"] for n in (64, 256, 257, 4160)] == [64, 256, 257, 4160] and 4160 % 64 == 0 and 4160 % 256 != 0
    for m in ec.PROJ_M:                                              # R is dense beyond the identity: every row of V is read
        g = case("proj_m%d" % m)
        assert m == g["base_sel"] or np.count_nonzero(g["R"][:, g["base_sel"]:]) > 0.8 * g["R"][:, g["base_sel"]:].size
    # all 16 rows
    for name, m in (("rows16_m16", 16), ("rows16_m37", 37)):
        g = case(name)
        assert g["base_sel"] == 16 and g["m"] == m and g["n"] == 1061 and len(cc.pairs(16)) == 120
        assert len(set(r.tobytes() for r in g["P"])) == 16
    assert np.array_equal(case("rows16_m16")["hull"], case("rows16_m37")["hull"])
    # the panel loop
    pan = case("panel_8x65600")
    assert (pan["m"], pan["n"]) == (8, 65600) and pan["n"] // 64 == 1025
    assert list(pan["hull"]) == list(ec.PANEL_CORNERS) and ec.PANEL_CORNERS[1] < 64 and ec.PANEL_CORNERS[2] >= 65600 - 64
    assert len(_survivors(pan, 0, 1, cc.D0)) == 4
    # the forced-capacity runs: more survivors than the forced capacity with both numbers of directions
    for name in ec.FORCED_CAP_CASES:
        g = case(name)
        for i, j in cc.pairs(g["base_sel"]):
            assert min(len(_survivors(g, i, j, cc.D0)), len(_survivors(g, i, j, cc.D1))) > ec.FORCED_CAP
