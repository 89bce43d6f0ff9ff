"""pymf_amd.CHNMF and pmf_chnmf_hull on the MI355X against the goldens of the real pymf/chnmf.py (tests/golden/chnmf_*.npz,
tests/chnmf_cases.py).  The fixtures are determinate (tests/test_chnmf_cases.py): `_hull_idx` must be the reference's exactly.

W, H and ferr: the nested AA runs 50 alternating iterations from a random start; the existing AA tests hold one iteration from
a fixed start to the float64 oracle (tests/test_gpu_aa.py: test_parity) and establish that two runs from one start give the
same bits (test_hooks_by_hand_equal_factorize_and_second_run_same_bits) -- they make no statement about 50 iterations against
a float64 run.  What they make determinate, and what is asserted here, is the second alternative of the two: W is bit-equal
to pymf_amd.AA run on data[:, _hull_idx] from the same start, H and ferr bit-equal to AA's H step and error on the full data
with that W.  The distances to the golden's W, H and ferr are printed, not asserted."""
import numpy as np
import pytest

import pymf_amd
import chnmf_cases as cc
from conftest import rel_fro
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

_runs = {}


def hull_cabi(name, survivor_cap=0, max_wgs=0):
    g = cc.fixture(name)
    m, n = g["V"].shape
    ctx = _lib.Context(_lib.ALGO_AA, m, n, g["k"])
    ctx.set_v_dense(g["V"])
    ctx.chnmf_set_limits(survivor_cap, max_wgs)
    idx = ctx.chnmf_hull(g["R"])
    routes = ctx.chnmf_routes()
    ctx.close()
    return idx, routes


def device(name):
    """One seeded factorize() of the fixture through the class, kept for the tests that only read it."""
    if name not in _runs:
        g = cc.fixture(name)
        np.random.seed(g["seed"])
        mdl = pymf_amd.CHNMF(g["V"].copy(), num_bases=g["k"], base_sel=3 if name == "chnmf_doc_2x3_k2" else g["base_sel"])
        mdl.factorize()
        _runs[name] = mdl
    return cc.fixture(name), _runs[name]


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_cabi_hull_is_the_references(name):
    g = cc.fixture(name)
    idx, routes = hull_cabi(name)
    assert idx.dtype == np.int32
    assert np.array_equal(idx, g["_hull_idx"]), (idx, g["_hull_idx"])
    assert routes == (len(cc.pairs(g["base_sel"])), 0, 0)      # every pair ended on the 32-direction filter and the device chain
    again, _ = hull_cabi(name)
    assert again.tobytes() == idx.tobytes()
    if name == cc.DUPS:
        assert set(int(v) for v in g["dup_vertices"]) <= set(int(v) for v in idx)


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_class_under_the_fixtures_seed(name):
    g, mdl = device(name)
    V = g["V"]
    assert mdl._base_sel == g["base_sel"]
    assert np.array_equal(mdl._hull_idx, g["_hull_idx"]) and mdl._hull_idx.dtype == np.int32
    assert mdl.W.shape == g["W"].shape and mdl.H.shape == g["H"].shape and len(mdl.ferr) == 1
    print("%s  to the golden: W %.3e  H %.3e  ferr %.3e" % (name, float(rel_fro(mdl.W, g["W"], name + " W (printed)")),
                                                           float(rel_fro(mdl.H, g["H"], name + " H (printed)")),
                                                           abs(mdl.ferr[0] - g["ferr"][0]) / g["ferr"][0]))
    # the same start: the reference's draws in its order -- R, then the nested AA's init_w (beta, W) and init_h (H)
    np.random.seed(g["seed"])
    np.random.randn(g["base_sel"], V.shape[0])
    sub = pymf_amd.AA(np.ascontiguousarray(V[:, g["_hull_idx"]]), num_bases=g["k"])
    sub.factorize(niter=50)
    assert np.array_equal(np.asarray(mdl.W), np.asarray(sub.W))
    full = pymf_amd.AA(V.copy(), num_bases=g["k"])
    full.W = np.array(sub.W)
    full.H = np.zeros((g["k"], V.shape[1]))
    full.factorize(niter=1, compute_w=False)
    assert np.array_equal(np.asarray(mdl.H), np.asarray(full.H)) and mdl.ferr[0] == full.ferr[0]
    # _map_w_to_data: the nearest data column of every base, float64 distances from the returned W
    W64, V64 = np.asarray(mdl.W, dtype=np.float64), V.astype(np.float64)
    want = [int(np.argmin(((V64 - W64[:, i:i + 1]) ** 2).sum(axis=0))) for i in range(g["k"])]
    assert list(mdl._Wmapped_index) == want
    assert np.array_equal(mdl.Wmapped, V64[:, want])


def test_two_runs_same_bits():
    g, mdl = device("chnmf_37x1061_k5_sel5")
    np.random.seed(g["seed"])
    again = pymf_amd.CHNMF(g["V"].copy(), num_bases=g["k"], base_sel=g["base_sel"])
    again.factorize()
    assert again._hull_idx.tobytes() == mdl._hull_idx.tobytes()
    assert np.array_equal(again.W, mdl.W) and np.array_equal(again.H, mdl.H) and again.ferr[0] == mdl.ferr[0]


@pytest.mark.parametrize("max_wgs", [1, 3, 1024])
def test_panel_ranges(max_wgs):
    """n = 5000 is 79 panels: one workgroup owning all of them, three owning 27, 27 and 25, and one panel per workgroup."""
    g = cc.fixture(cc.RING)
    idx, routes = hull_cabi(cc.RING, max_wgs=max_wgs)
    assert np.array_equal(idx, g["_hull_idx"]) and routes == (1, 0, 0)


def test_capacity_routes():
    """The ring: 400 vertices and a few near-hull points survive 32 directions, the vertices alone 128 directions."""
    g = cc.fixture(cc.RING)
    P = cc.proj64(g["V"], g["R"])
    s32, s128 = len(cc.filter_survivors(P[0], P[1], cc.D0)), len(cc.filter_survivors(P[0], P[1], cc.D1))
    print("survivors: %d with 32 directions, %d with 128" % (s32, s128))
    assert 64 < s128 < s32 <= cc.CAP
    idx, routes = hull_cabi(cc.RING, survivor_cap=64)          # too many both times: the rerun runs, then the host forms the hull
    assert np.array_equal(idx, g["_hull_idx"]) and routes == (0, 0, 1)
    idx, routes = hull_cabi(cc.RING, survivor_cap=s128)        # the rerun's survivors fit
    assert np.array_equal(idx, g["_hull_idx"]) and routes == (0, 1, 0)


def test_refusals_on_the_device():
    g = cc.fixture("chnmf_29x300_k6_sel3")
    m, n = g["V"].shape
    ctx = _lib.Context(_lib.ALGO_AA, m, n, g["k"])
    with pytest.raises(_lib.PmfError, match="V has not been set"):
        ctx.chnmf_hull(g["R"])
    ctx.set_v_dense(g["V"])
    with pytest.raises(_lib.PmfError, match="base_sel"):
        ctx.chnmf_hull(np.zeros((17, m)))
    with pytest.raises(_lib.PmfError, match="survivor_cap"):
        ctx.chnmf_set_limits(4097, 0)
    ctx.close()
    ctx = _lib.Context(_lib.ALGO_SIVM, m, n, g["k"])
    ctx.set_v_dense(g["V"])
    with pytest.raises(_lib.PmfError, match="AA contexts only"):
        ctx.chnmf_hull(g["R"])
    ctx.close()
