"""The CHNMF fixtures are determinate and the device's stage 2, restated in NumPy, gives the reference's hull on them
(tests/chnmf_cases.py).  No GPU."""
import re
import os

import numpy as np
import pytest

import chnmf_cases as cc
from conftest import ROOT


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_fixture_is_determinate(name):
    g = cc.fixture(name)
    assert g["R"].shape == (g["base_sel"], g["V"].shape[0]) and g["R"].dtype == np.float64 and g["V"].dtype == np.float32
    np.random.seed(g["seed"])
    assert np.array_equal(np.random.randn(*g["R"].shape), g["R"])          # R is the seed's first draw
    outer, inner, sep, tau = cc.margins(g["V"], g["R"])
    print("%s  vertex margin %.3e  interior margin %.3e  separation %.3e  tau %.3e" % (name, outer, inner, sep, tau))
    assert tau == 1e4 * cc.gamma(g["V"], g["R"])
    assert outer > tau
    assert inner > tau
    assert sep > tau


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_strict_monotone_chain_gives_the_references_hull(name):
    g = cc.fixture(name)
    hull = g["_hull_idx"]
    assert hull.dtype == np.int32 and np.all(np.diff(hull) > 0)
    assert np.array_equal(cc.hull_union(g["V"], g["R"]), hull)


@pytest.mark.parametrize("name", cc.FIXTURES)
@pytest.mark.parametrize("D", [cc.D0, cc.D1])
def test_filter_keeps_every_vertex(name, D):
    g = cc.fixture(name)
    P = cc.proj64(g["V"], g["R"])
    for i, j in cc.pairs(g["base_sel"]):
        surv = cc.filter_survivors(P[i], P[j], D)
        verts = cc.chain_hull(P[i], P[j])
        assert set(verts) <= set(int(s) for s in surv)
        assert cc.chain_hull(P[i][surv], P[j][surv], surv) == verts


def test_what_the_fixtures_are_for():
    ring = cc.fixture(cc.RING)
    P = cc.proj64(ring["V"], ring["R"])
    assert ring["V"].shape == (8, 5000) and len(ring["_hull_idx"]) >= 200
    assert len(cc.filter_survivors(P[0], P[1], cc.D0)) > 64
    wide = cc.fixture("chnmf_37x1061_k5_sel5")
    assert wide["V"].shape[1] % 64 != 0 and wide["V"].shape[0] % 4 != 0 and len(cc.pairs(wide["base_sel"])) == 10
    doc = cc.fixture("chnmf_doc_2x3_k2")
    assert doc["base_sel"] == 2 and list(doc["_hull_idx"]) == [0, 1, 2]    # base_sel = 3 clipped to the two rows
    dups = cc.fixture(cc.DUPS)
    cols = {}
    for c in range(dups["V"].shape[1]):
        cols.setdefault(dups["V"][:, c].tobytes(), []).append(c)
    groups = [grp for grp in cols.values() if len(grp) > 1]
    assert len(groups) == 10
    on_hull = [grp for grp in groups if set(grp) & set(int(h) for h in dups["_hull_idx"])]
    assert len(on_hull) >= 2 and sorted(min(grp) for grp in on_hull) == sorted(int(v) for v in dups["dup_vertices"])
    for grp in on_hull:                                                    # the lowest index, and it alone
        assert [c for c in grp if c in set(int(h) for h in dups["_hull_idx"])] == [min(grp)]


def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_chnmf.h")).read()

    def constant(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert (cc.CAP, cc.D0, cc.D1) == (constant("PMF_CH_CAP"), constant("PMF_CH_D0"), constant("PMF_CH_D1"))
    d = cc.directions(cc.D1)
    assert np.array_equal(d[[0, 32, 64, 96]], [[1, 0], [0, 1], [-1, 0], [0, -1]])
    assert np.array_equal(cc.directions(cc.D0), d[::4])
