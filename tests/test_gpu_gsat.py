"""pymf_amd.SIVM_GSAT on the MI355X against the reference goldens (tests/golden/gen_golden_gsat.py) and the float64 twin
(tests/gsat_oracle.py) on the cases of tests/gsat_cases.py.  Verdicts, select and W must be exact.  _v and V: 1e-10 against the
twin with the exact f1 (float64 with another summation order), 1e-07 against the goldens, whose f1 carries the reference's
float32 roundings (gsat_cases.py).  The 64-base case has no golden -- the reference's f1 is 0 from 20 bases on -- and is held
against the twin alone.  The achieved errors are written as parity_gsat.json next to the session's parity ledger (conftest.LEDGER_PATH) and committed
as profiles/parity_gsat.json."""
import json
import os

import numpy as np
import pytest

import gsat_cases as gc
import gsat_oracle as go
import pymf_amd
from conftest import LEDGER_PATH, close, load_golden, rel_fro

pytestmark = pytest.mark.gpu

_ACHIEVED = {}


def record(name, **figures):
    _ACHIEVED.setdefault(name, {}).update({k: float(v) for k, v in figures.items()})
    try:
        out_dir = os.path.dirname(LEDGER_PATH)
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "parity_gsat.json"), "w") as f:
            json.dump({"bounds": {"v_against_twin": gc.TWIN_V_TOL, "v_against_golden": gc.GOLDEN_V_TOL}, "achieved": _ACHIEVED}, f, indent=1, sort_keys=True)
    except OSError:
        pass


def rel_v(got, want):
    assert len(got) == len(want), (len(got), len(want))
    return max([abs(a - b) / b for a, b in zip(got, want)] or [0.0])


def walk(name, **kw):
    s = gc.spec(name)
    mdl = pymf_amd.SIVM_GSAT(gc.data(name), num_bases=s["k"], dist_measure=s["measure"])
    np.random.seed(s["seed"])
    kw.setdefault("niter", s["niter"])
    mdl.factorize(compute_h=False, compute_err=False, **kw)
    return s, mdl


def check_against(name, mdl, want_select, want_W, want_v, want_V, tol, what):
    assert type(mdl.select) is list and mdl.select == [int(x) for x in want_select]
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float64), want_W)
    assert type(mdl._v) is list and all(type(v) is float for v in mdl._v)
    dv, dV = rel_v(mdl._v, want_v), abs(mdl.V - want_V) / want_V
    print("%s against %s: _v %.3e V %.3e (bound %.1e), %d swaps" % (name, what, dv, dV, tol, len(mdl._v) - 1))
    record(name, **{"v_against_" + what: dv, "V_against_" + what: dV})
    assert dv <= tol and dV <= tol
    assert mdl._v[-1] == mdl.V


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_walk_parity(name):
    s, mdl = walk(name)
    t = gc.twin(name)
    assert np.array_equal(mdl._last_slots, t["slots"])
    check_against(name, mdl, t["select"], t["W"], t["v"], t["V"], gc.TWIN_V_TOL, "twin")
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), gc.data(name)[:, mdl.select])     # bit-exact data columns
    if name in gc.GOLDEN_CASES:
        g = load_golden(name)
        assert np.array_equal(mdl._last_slots, g["slots"])
        check_against(name, mdl, g["select"], g["W"], g["v"], float(g["vol"]), gc.GOLDEN_V_TOL, "golden")
    D = mdl.D
    assert D.shape == (s["k"] + 1, s["k"] + 1) and D.dtype == np.float64
    assert rel_fro(D, t["D"], name + " D") <= gc.TWIN_V_TOL


def test_doc_cases():
    g = load_golden("gsat_doc_2x3_k2")
    mdl = pymf_amd.SIVM_GSAT(g["V"], num_bases=2)
    np.random.seed(int(g["seed"]))
    mdl.factorize()
    assert mdl.select == [int(x) for x in g["select"]] and np.array_equal(np.asarray(mdl.W, dtype=np.float64), g["W"])
    assert rel_v(mdl._v, g["v"]) <= gc.GOLDEN_V_TOL
    close(mdl.H, g["H"], rtol=0, atol=1e-6, what="gsat doc H")
    assert abs(mdl.ferr[0] - g["ferr"][0]) <= 1e-6 * max(1.0, g["ferr"][0])
    u = load_golden("gsat_doc_userw")
    mdl = pymf_amd.SIVM_GSAT(u["V"], num_bases=2)
    mdl.W = u["W"].copy()
    mdl.factorize(compute_w=False)
    assert np.array_equal(mdl.W, u["W"]) and not hasattr(mdl, "select")
    close(mdl.H, u["H"], rtol=0, atol=1e-6, what="gsat userw H")
    assert abs(mdl.ferr[0] - u["ferr"][0]) <= 1e-6


def test_degenerate_more_bases_than_dimension_plus_one():
    """rows + 1 < k: every volume is rounding noise (in the reference too).  Only validity is asked."""
    name = "gsat_16x120_k20"
    s, mdl = walk(name)
    slots = mdl._last_slots
    assert len(slots) == s["niter"] and all(-2 <= int(x) < s["k"] for x in slots)
    assert len(set(mdl.select)) == s["k"] and all(type(x) is int and 0 <= x < s["n"] for x in mdl.select)
    assert np.isfinite(mdl.W).all()
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), gc.data(name)[:, mdl.select])
    assert mdl.select == _replay(gc.draws(name), slots, s["k"])


def _replay(idx, slots, k):
    sel = list(range(k))
    for n, x in zip(idx, slots):
        if x >= 0:
            sel[int(x)] = int(n)
    return sel


def test_online_update_w_with_vectors_that_are_no_data_columns():
    """One accepted, one rejected, one equal to a current vertex, against the twin.  The vertex's own volume v[j] and V are
    the same determinant up to a permutation of rows and columns: which of the two is larger is rounding noise in any float64
    implementation, the reference's included, so that probe may end as a reject or as the swap of vertex j with its equal --
    W, V and D are the same either way, and they are what is compared."""
    name = "gsat_29x300_k6_l2"
    s = gc.spec(name)
    V = gc.data(name)
    mdl = pymf_amd.SIVM_GSAT(V, num_bases=s["k"])
    mdl.init_w()
    tw = go.Walk(V.astype(np.float64), s["k"])
    far = (V[:, 0] + 40.0 * (np.arange(s["m"]) % 3 - 1)).astype(np.float32)      # far outside the data: accepted
    inside = V[:, :s["k"]].mean(axis=1).astype(np.float32)                         # the barycentre of the vertices: rejected
    for vec, accepted in ((far, True), (inside, False)):
        got, want = mdl.online_update_w(vec), tw.online_update_w(vec.astype(np.float64))
        assert got == want and got[0] is accepted and type(got[1]) is int
        assert np.array_equal(np.asarray(mdl.W, dtype=np.float64), tw.W)
        assert abs(mdl.V - tw.V) <= gc.TWIN_V_TOL * tw.V
    assert rel_v(mdl._v, tw._v) <= gc.TWIN_V_TOL
    assert mdl.select == list(range(s["k"]))                                       # online_update_w leaves `select` alone
    j = 2
    W_before, V_before = np.array(mdl.W), mdl.V
    updated, slot = mdl.online_update_w(np.array(mdl.W[:, j]))
    assert (updated, slot) in ((False, -1), (True, j))
    assert np.array_equal(mdl.W, W_before) and abs(mdl.V - V_before) <= gc.TWIN_V_TOL * V_before
    assert rel_fro(mdl.D[:s["k"], :s["k"]], tw.D[:s["k"], :s["k"]], "gsat D after an equal vertex") <= gc.TWIN_V_TOL


def test_walk_from_an_sgreedy_selection():
    name = "gsat_29x300_k6_l2"
    s = gc.spec(name)
    V = gc.data(name)
    start = pymf_amd.SIVM_SGREEDY(V, num_bases=s["k"])
    start.update_w()
    idx = gc.draws(name)[:300]
    t = go.walk(V.astype(np.float64), s["k"], idx, W=np.asarray(start.W, dtype=np.float64), select=start.select)
    mdl = pymf_amd.SIVM_GSAT(V, num_bases=s["k"])
    mdl.W, mdl.select = np.array(start.W), list(start.select)
    np.random.seed(s["seed"])
    mdl.factorize(niter=300, compute_h=False, compute_err=False)
    assert np.array_equal(mdl._last_slots, t["slots"]) and mdl.select == t["select"]
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float64), t["W"])
    assert abs(mdl.V - t["V"]) <= gc.TWIN_V_TOL * t["V"] and rel_v(getattr(mdl, "_v", []), t["v"]) <= gc.TWIN_V_TOL
    assert mdl.V >= go.cmdet(go.pdist(np.asarray(start.W, dtype=np.float64))) * (1.0 - gc.TWIN_V_TOL)   # the walk never loses volume


def test_one_call_walk_equals_single_probes_and_repeats_bit_for_bit():
    name = "gsat_29x300_k6_l1"
    s, a = walk(name, niter=300)
    b = pymf_amd.SIVM_GSAT(gc.data(name), num_bases=s["k"], dist_measure=s["measure"])
    b.init_w()
    np.random.seed(s["seed"])
    for _ in range(300):
        b.update_w()
    assert a.select == b.select and a._v == b._v and a.V == b.V
    assert np.array_equal(a.W, b.W)
    _, c = walk(name, niter=300)
    assert c.select == a.select and c._v == a._v and c.V == a.V and np.array_equal(c.W, a.W)
    assert np.array_equal(c._last_slots, a._last_slots)


def test_factorize_with_h_and_ferr_against_the_golden():
    g = load_golden(gc.H_CASE + "_h")
    s = gc.spec(gc.H_CASE)
    mdl = pymf_amd.SIVM_GSAT(gc.data(gc.H_CASE), num_bases=s["k"])
    np.random.seed(s["seed"])
    mdl.factorize(niter=3)
    assert mdl.select == [int(x) for x in g["select"]] and np.array_equal(np.asarray(mdl.W, dtype=np.float64), g["W"])
    assert rel_v(mdl._v, g["v"]) <= gc.GOLDEN_V_TOL
    import sgreedy_cases as sg
    assert mdl.ferr.shape == (3,) and np.asarray(mdl.H).dtype == np.float64
    assert rel_fro(mdl.H, g["H"], "gsat golden H") <= sg.H_TOL
    close(mdl.ferr, g["ferr"], rtol=sg.FERR_TOL, what="gsat golden ferr")


def test_option_refusals():
    from pymf_amd import _lib
    ctx = _lib.Context(_lib.ALGO_NMF, 64, 64, 4)
    try:
        with pytest.raises(_lib.PmfError, match="sivm_gsat: SIVM contexts only"):
            ctx.set_option("sivm_gsat", 1)
    finally:
        ctx.close()
    ctx = _lib.Context(_lib.ALGO_SIVM, 8, 64, 2)
    try:
        with pytest.raises(_lib.PmfError, match="under sivm_gsat only"):
            ctx.gsat_walk([1])
        for rule in (1, 2):
            ctx.set_option("sivm_rule", rule)
            with pytest.raises(_lib.PmfError, match="not together with"):
                ctx.set_option("sivm_gsat", 1)
        ctx.set_option("sivm_rule", 0)
        ctx.set_option("sivm_sgreedy", 1)
        with pytest.raises(_lib.PmfError, match="not together with"):
            ctx.set_option("sivm_gsat", 1)
        ctx.set_option("sivm_sgreedy", 0)
        ctx.set_option("sivm_gsat", 1)
        for name, value in (("sivm_rule", 1), ("sivm_rule", 2), ("sivm_sgreedy", 1)):
            with pytest.raises(_lib.PmfError, match="not together with sivm_gsat"):
                ctx.set_option(name, value)
        ctx.set_v_dense(np.ones((8, 64), dtype=np.float32))
        ctx.set_w(np.eye(8, 2))
        with pytest.raises(_lib.PmfError, match="pmf_gsat_start"):
            ctx.gsat_walk([1])
        with pytest.raises(_lib.PmfError, match="no W step of its own"):
            ctx.update_w()
        ctx.gsat_start([0, 1])
        with pytest.raises(_lib.PmfError, match="outside"):
            ctx.gsat_walk([64])
    finally:
        ctx.close()
