"""The cases of tests/vq_cases.py without a GPU: the builders' own invariants, the integer expectations against the REAL
pymf/dist.py recorded in tests/golden/vq_exact.npz (tests/golden/gen_golden_vq.py), the float64 restatement of the generic
cases against tests/golden/vq_generic.npz, the 95 % condition, and the constants against the kernel's header."""
import os
import re

import numpy as np
import pytest

import vq_cases as vc
from conftest import GOLDEN, ROOT

SMALL = [s for s in vc.exact_shapes() if s[1] <= 257]


def header_constant(name):
    text = open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_vq.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_constants_are_the_headers():
    assert vc.TILE == header_constant("PMF_VQ_TILE")
    assert vc.MAX_Q == header_constant("PMF_VQ_MAX_Q")
    assert vc.LDS_FLOATS == header_constant("PMF_VQ_LDS")
    text = open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_cluster.h")).read()
    assert vc.MAX_WGS == int(re.search(r"constexpr int PMF_CL_MAX_WGS = (\d+);", text).group(1))


def test_the_shapes_are_the_issues():
    shapes = vc.exact_shapes()
    assert {s[0] for s in shapes} == {1, 3, 4, 5, 7, 64, 65}
    assert {s[1] for s in SMALL} == {1, 63, 64, 65, 257}
    assert {s[2] for s in SMALL} == {1, 15, 16, 17, 64, 65, 128}
    assert len(SMALL) == 7 * 5 * 7
    # the deep shapes: one column past 1024 ranges of 1, 4 and 16 panels -- 2, 5 and 17 panels per workgroup
    assert [vc.partition(n)[0] // 64 for _, n, _ in vc.DEEP] == [2, 5, 17]
    assert vc.partition(65536) == (64, 1024) and vc.partition(65) == (64, 2) and vc.partition(1) == (64, 1)


def test_exact_cases_are_exact_and_reach_their_edges():
    """exact_case asserts every planted tie while it builds; here: the bounds, and that the boundaries of the sweep are reached
    by some case: quad, panel = workgroup, last column, wave and trip inside a range, a tile of queries, the zero query."""
    edges = set()
    for s in vc.exact_shapes():
        c = vc.exact(*s)
        assert np.array_equal(c.V.astype(np.int64), c.Vi) and np.array_equal(c.Q.astype(np.int64), c.Qi)
        assert int(np.abs(c.Vi).max()) <= 64 and int(np.abs(c.Qi).max()) <= 64 and c.m <= 65
        wg_cols, wgs = vc.partition(c.n)
        for a, b, _ in c.col_ties:
            assert b == a + 1
            edges.update(tag for tag, hit in (("quad", b % 4 == 0), ("panel", b % 64 == 0), ("wave", b % 256 == 0 and b % wg_cols),
                                              ("trip", b % 1024 == 0 and b % wg_cols), ("workgroup", b % wg_cols == 0),
                                              ("last", b == c.n - 1), ("wide workgroup", b % wg_cols == 0 and wg_cols > 64)) if hit)
        for _, j1, j2 in c.asg_ties:
            edges.update(tag for tag, hit in (("query tile", j2 % vc.TILE == 0 and j1 == j2 - 1), ("query ends", j1 == 0 and j2 == c.nq - 1)) if hit)
        if c.zero_q is not None:
            edges.add("zero query")
        if c.nq >= 2 and c.n >= 3:
            assert c.asg_ties and (c.col_ties or c.nq == 2), c.name
    assert edges == {"quad", "panel", "wave", "trip", "workgroup", "wide workgroup", "last", "query tile", "query ends", "zero query"}


def test_squared_recovers_the_integers():
    """The widened float32 root of an exact integer below 2^21, squared in float64, rounds back to that integer."""
    c = vc.exact(65, 257, 128)
    root = np.sqrt(c.D2.astype(np.float32)).astype(np.float64)
    assert np.array_equal(c.squared("l2", root), c.D2)
    bumped = np.nextafter(np.sqrt(c.D2.astype(np.float32)), np.float32(np.inf)).astype(np.float64)     # (one unit off: still the integer)
    assert np.array_equal(c.squared("l2", bumped), c.D2)
    assert np.array_equal(c.squared("l1", c.D1.astype(np.float64)), c.D1)


@pytest.fixture(scope="module")
def gold_exact():
    return np.load(os.path.join(GOLDEN, "vq_exact.npz"))


@pytest.fixture(scope="module")
def gold_generic():
    return np.load(os.path.join(GOLDEN, "vq_generic.npz"))


def test_integer_expectations_are_the_references(gold_exact):
    """vq both ways and pdist of the real pymf.dist on every small exact case equal the integer arithmetic: array_equal."""
    seen_pd = 0
    for s in SMALL:
        c = vc.exact(*s)
        for k in vc.METRICS:
            assert np.array_equal(gold_exact["%s/cols_%s" % (c.name, k)], c.cols[k]), (c.name, k)
            assert np.array_equal(gold_exact["%s/asg_%s" % (c.name, k)], c.asg[k]), (c.name, k)
            key = "%s/pd_%s" % (c.name, k)
            if key in gold_exact.files:
                seen_pd += 1
                pd = gold_exact[key]
                assert np.array_equal(c.squared(k, pd), c.D[k]), (c.name, k)
                if k == "l2":
                    assert np.array_equal(pd, np.sqrt(c.D2.astype(np.float64)))
    assert seen_pd == 2 * 3 * 4 * 4                     # m in (1, 4, 65), n in (1, 63, 64, 65), nq in (1, 15, 16, 17)
    assert len(gold_exact.files) == 4 * len(SMALL) + seen_pd


@pytest.mark.parametrize("name", sorted(vc.generic_specs()))
def test_generic_restatement_is_the_reference(name, gold_generic):
    c = vc.generic(name)
    for k in vc.METRICS:
        pd = gold_generic["%s/pd_%s" % (name, k)]
        assert np.array_equal(pd, c.ref[k][:pd.shape[0], :pd.shape[1]]), (name, k)
        assert np.array_equal(gold_generic["%s/cols_%s" % (name, k)], np.argmin(c.ref[k], axis=1))
        assert np.array_equal(gold_generic["%s/asg_%s" % (name, k)], np.argmin(c.ref[k], axis=0))


@pytest.mark.parametrize("name", sorted(vc.generic_specs()))
def test_generic_cases_lie_above_the_gap(name):
    """At least 95 % of the decisions of every generic case, both metrics and both directions, are decided by more than 2 EPS --
    by the reference alone; and the checkers accept the reference itself and refuse a wrong index and a distance 2 EPS off."""
    c = vc.generic(name)
    assert c.eps == (c.m + 4) * 2.0 ** -24
    for k in vc.METRICS:
        for tag in ("cols", "asg"):
            assert c.above[k, tag].mean() >= 0.95, (name, k, tag)
        cols, asg = np.argmin(c.ref[k], axis=1), np.argmin(c.ref[k], axis=0)
        assert c.check_index(k, "cols", cols) and c.check_index(k, "asg", asg)
        assert c.check_dist(k, c.ref[k]) == 0.0
        assert c.check_dist(k, c.ref[k] * (1.0 + 2.0 * c.eps)) > 1.0
        wrong = cols.copy()
        wrong[0] = (wrong[0] + 1) % c.n
        assert not c.check_index(k, "cols", wrong)
    spec = vc.generic_specs()
    assert sorted(v[0] for v in spec.values())[-2:] == [300, 1100] and any(v[4] == 1e3 for v in spec.values())
    assert any(v[0] > vc.LDS_FLOATS // vc.TILE for v in spec.values())                      # more than one slab of rows
    assert any(v[0] * ((v[2] + 15) // 16 * 16) > vc.LDS_FLOATS for v in spec.values())      # the tile-at-a-time form is reached
