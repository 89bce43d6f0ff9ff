"""pymf_amd.SIVM_SGREEDY on the MI355X against the literal float64 oracle (tests/sgreedy_oracle.py) on the cases of
tests/sgreedy_cases.py and against the reference goldens.  select and W must be exact; _v, H and ferr within the tolerances
that sgreedy_cases derives from the float32 twin's own error (4 x the measured worst)."""
import numpy as np
import pytest

import sgreedy_cases as gc
import pymf_amd
from conftest import close, load_golden, rel_fro
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN_CASES = ["sgreedy_29x300_k6_l2", "sgreedy_29x300_k6_l1", "sgreedy_29x300_k6_cosine", "sgreedy_29x300_k6_origin"]


def model(name):
    c = gc.case(name)
    return c, pymf_amd.SIVM_SGREEDY(c["V"], num_bases=c["k"], dist_measure=c["metric"], init=c["init"])


def device(name, **kw):
    c, mdl = model(name)
    mdl.factorize(**kw)
    return c, mdl


def check_select_w_v(name, c, mdl):
    print("%s select %s" % (name, mdl.select))
    assert mdl.select == c["select"]
    assert all(type(s) is int for s in mdl.select)
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), c["V"][:, c["select"]])
    assert type(mdl._v) is list and len(mdl._v) == c["k"] - 1 and all(type(v) is float for v in mdl._v)
    dv = max([abs(a - b) / b for a, b in zip(mdl._v, c["v"])] or [0.0])
    print("%s _v deviation %.3e (tol %.3e)" % (name, dv, gc.V_TOL))
    assert dv <= gc.V_TOL
    assert len(mdl._t) == c["k"] - 1 and all(type(t) is float and t >= 0.0 for t in mdl._t)
    assert all(a <= b for a, b in zip(mdl._t, mdl._t[1:]))


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_parity(name):
    c, mdl = device(name)
    check_select_w_v(name, c, mdl)
    H = np.asarray(mdl.H)
    assert H.dtype == np.float64 and H.shape == c["H"].shape
    dh = rel_fro(H, c["H"], name + " H")
    df = abs(mdl.ferr[0] - c["ferr"]) / c["ferr"]
    print("%s H deviation %.3e (tol %.3e)  ferr deviation %.3e (tol %.3e)  min H %.3e  max |sum - 1| %.3e" % (
        name, float(dh), gc.H_TOL, df, gc.FERR_TOL, H.min(), np.abs(H.sum(axis=0) - 1.0).max()))
    assert dh <= gc.H_TOL
    close(mdl.ferr[0], c["ferr"], rtol=gc.FERR_TOL, what=name + " ferr")
    assert H.min() >= 0.0
    assert np.abs(H.sum(axis=0) - 1.0).max() <= 1e-5


@pytest.mark.parametrize("name", sorted(gc.PANEL_CASES))
def test_panel_ranges_select_and_w(name):
    """Several panels per workgroup and the second trip of the quad loop: selection and W only (sgreedy_cases.py)."""
    c, mdl = device(name, compute_h=False, compute_err=False)
    assert mdl.select == c["select"]
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), c["V"][:, c["select"]])


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_parity(name):
    """The same cases against what the reference itself wrote (tests/golden/gen_golden_sgreedy.py)."""
    g = load_golden(name)
    c, mdl = device(name)
    assert mdl.select == [int(s) for s in g["select"]]
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float64), g["W"])
    assert max(abs(a - b) / b for a, b in zip(mdl._v, g["v"])) <= gc.V_TOL
    assert rel_fro(mdl.H, g["H"], name + " golden H") <= gc.H_TOL
    close(mdl.ferr[0], g["ferr"][0], rtol=gc.FERR_TOL, what=name + " golden ferr")


@pytest.mark.parametrize("name", ["sgreedy_doc_2x3_k2", "sgreedy_37x29_k5"])
def test_small_goldens(name):
    g = load_golden(name)
    mdl = pymf_amd.SIVM_SGREEDY(g["V"], num_bases=int(g["k"]))
    mdl.factorize()
    assert mdl.select == [int(s) for s in g["select"]]
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float64), g["W"])
    assert max(abs(a - b) / b for a, b in zip(mdl._v, g["v"])) <= gc.V_TOL
    close(mdl.H, g["H"], rtol=0, atol=1e-6, what=name + " H")
    assert abs(mdl.ferr[0] - g["ferr"][0]) <= 1e-6 * max(1.0, g["ferr"][0])


def test_user_w_matches_golden():
    g = load_golden("sgreedy_doc_userw")
    mdl = pymf_amd.SIVM_SGREEDY(g["V"], num_bases=2)
    mdl.W = g["W"].copy()
    mdl.factorize(compute_w=False)
    assert np.array_equal(mdl.W, g["W"])
    close(mdl.H, g["H"], rtol=0, atol=1e-6, what="userw H")
    assert abs(mdl.ferr[0] - g["ferr"][0]) <= 1e-6


def test_hooks_by_hand_equal_factorize():
    c, ref = device("sgreedy_29x300_k6_l2")
    _, mdl = model("sgreedy_29x300_k6_l2")
    mdl.update_w()
    mdl.update_h()
    assert mdl.select == ref.select and mdl._v == ref._v
    assert np.array_equal(mdl.W, ref.W)
    assert np.array_equal(mdl.H, ref.H)
    assert mdl.frobenius_norm() == ref.ferr[0]


def test_second_factorize_same_bits():
    c, mdl = device("sgreedy_64x4113_k8")
    sel, v, W, H, ferr = list(mdl.select), list(mdl._v), np.array(mdl.W), np.array(mdl.H), mdl.ferr[0]
    mdl.factorize()
    assert mdl.select == sel and mdl._v == v
    assert np.array_equal(mdl.W, W) and np.array_equal(mdl.H, H) and mdl.ferr[0] == ferr


@pytest.mark.parametrize("init", ["fastmap", "origin"])
def test_one_base_runs_no_round(init):
    c = gc.case("sgreedy_29x300_k6_l2")
    mdl = pymf_amd.SIVM_SGREEDY(c["V"], num_bases=1, init=init)
    mdl.update_w()
    want = [-1] if init == "origin" else [gc.sg.start(c["V"].astype(np.float64), "l2", "fastmap")]
    assert mdl.select == want and mdl._v == [] and mdl._t == []
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), c["V"][:, want])


def context(name, sgreedy=1, metric=0, init=0):
    c = gc.case(name)
    ctx = _lib.Context(_lib.ALGO_SIVM, c["V"].shape[0], c["V"].shape[1], c["k"])
    ctx.set_v_dense(c["V"])
    ctx.set_option("sivm_metric", metric)
    ctx.set_option("sivm_init", init)
    ctx.set_option("sivm_sgreedy", sgreedy)
    return c, ctx


@pytest.mark.parametrize("name,metric,init", [("sgreedy_29x300_k6_l2", 0, 0), ("sgreedy_29x300_k6_origin", 0, 1), ("sgreedy_32x300_k9", 0, 0)])
def test_launch_counts_and_bytes(name, metric, init):
    """k - 1 launches of k_sgreedy_pass through the profile interface, bytes_per_launch the mean over the rounds of
    4 m np + 4 np + 4 (t - 1) np; the site of k_sivm_pass sees none of them."""
    c, ctx = context(name, 1, metric, init)
    try:
        ctx.profile_enable(True)
        ctx.update_w()
        stats = ctx.kernel_stats()
        print(name, stats["name"], stats["launches"], stats["bytes_per_launch"])
        assert ctx.get_select().tolist() == c["select"]
        assert stats["name"] == "k_sgreedy_pass" and stats["launches"] == c["k"] - 1
        m, np_ = c["V"].shape[0], -(-c["V"].shape[1] // 64) * 64
        total = 0.0
        for t in range(1, c["k"]):
            total += 4.0 * m * np_ + 4.0 * np_ + 4.0 * (t - 1) * np_
        assert stats["bytes_per_launch"] == total / (c["k"] - 1)
        ctx.set_option("sivm_sgreedy", 0)                      # back to SIVM's rule: its site starts from zero
        assert ctx.kernel_stats()["name"].startswith("k_sivm_pass<") and ctx.kernel_stats()["launches"] == 0
        ctx.profile_enable(False)
    finally:
        ctx.close()


def test_option_refusals():
    ctx = _lib.Context(_lib.ALGO_NMF, 64, 64, 4)
    try:
        with pytest.raises(_lib.PmfError, match="sivm_sgreedy: SIVM contexts only"):
            ctx.set_option("sivm_sgreedy", 1)
    finally:
        ctx.close()
    ctx = _lib.Context(_lib.ALGO_SIVM, 8, 64, 2)
    try:
        for value in (-1, 2):
            with pytest.raises(_lib.PmfError, match="sivm_sgreedy: 0 or 1"):
                ctx.set_option("sivm_sgreedy", value)
        with pytest.raises(_lib.PmfError, match="sivm_sgreedy only"):
            ctx.get_volumes()
        for rule in (1, 2):
            ctx.set_option("sivm_rule", rule)
            with pytest.raises(_lib.PmfError, match="not together with sivm_rule"):
                ctx.set_option("sivm_sgreedy", 1)
            ctx.set_option("sivm_sgreedy", 0)
        ctx.set_option("sivm_rule", 0)
        ctx.set_option("sivm_sgreedy", 1)
        for rule in (1, 2):
            with pytest.raises(_lib.PmfError, match="not together with sivm_sgreedy"):
                ctx.set_option("sivm_rule", rule)
        with pytest.raises(_lib.PmfError, match="0 \\(SIVM\\), 1 \\(LAESA\\) or 2 \\(GMAP\\)"):
            ctx.set_option("sivm_rule", 3)                     # (the option's own range and message stay)
        ctx.set_option("sivm_rule", 0)
        with pytest.raises(_lib.PmfError, match="no selection yet"):
            ctx.get_volumes()
    finally:
        ctx.close()


def test_sivm_select_keeps_sivms_rule():
    """pmf_sivm_select on a context under sivm_sgreedy answers as on a plain SIVM context (SIVM_CUR depends on it), and does
    not disturb the context's own selection or volumes."""
    import sivm_cases as sc
    s = sc.case("29x300_k6_origin")
    c, ctx = context("sgreedy_29x300_k6_origin", 1, 0, 1)
    try:
        assert np.array_equal(c["V"], s["V"])
        ctx.update_w()
        v = ctx.get_volumes().tolist()
        assert ctx.get_select().tolist() == c["select"]
        assert ctx.sivm_select(s["k"], False, 0, 1, path=1).tolist() == s["select"]
        assert ctx.get_select().tolist() == c["select"] and ctx.get_volumes().tolist() == v
    finally:
        ctx.close()


def test_other_rules_are_unaffected():
    """SIVM, LAESA and GMAP contexts on the shared 29 x 300 data select what their own oracles say, before and after a
    SIVM_SGREEDY model has run on the same data."""
    import colsel_cases as cc
    import sivm_cases as sc

    def others():
        s = sc.case("29x300_k6_l2")
        a = pymf_amd.SIVM(s["V"], num_bases=s["k"])
        a.update_w()
        l = cc.case("laesa_29x300_k6_l2")
        b = pymf_amd.LAESA(l["V"], num_bases=l["k"])
        b.update_w()
        g = cc.case("gmap_29x300_k6_pca")
        d = pymf_amd.GMAP(g["V"], num_bases=g["k"], method="pca", robust_map=False)
        d.update_w()
        assert a.select == s["select"] and b.select == l["select"] and d.select == g["select"]
        return a.select, b.select, d.select

    before = others()
    c, mdl = device("sgreedy_29x300_k6_l2", compute_h=False, compute_err=False)
    assert np.array_equal(c["V"], sc.case("29x300_k6_l2")["V"])
    assert others() == before


def test_degenerate_more_bases_than_dimension():
    """5 x 300 data, 8 bases: from the seventh pick on the selected columns are affinely dependent and every volume is rounding
    noise, in the reference too.  The selection still returns eight in-range indices and a finite W, without an error."""
    V = gc.data(5, 300, 3, 11, None)[0]
    mdl = pymf_amd.SIVM_SGREEDY(V, num_bases=8)
    mdl.update_w()
    assert len(mdl.select) == 8 and all(type(s) is int and 0 <= s < 300 for s in mdl.select)
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), V[:, mdl.select]) and np.isfinite(mdl.W).all()
    assert len(mdl._v) == 7
