"""pymf_amd.LAESA and pymf_amd.GMAP on the MI355X against the float64 oracle (tests/colsel_oracle.py) on the cases of
tests/colsel_cases.py and against the reference goldens.  select and W must be exact; H and ferr within the tolerances that
colsel_cases derives from the oracle's own float32 error (4 x the measured worst)."""
import numpy as np
import pytest

import colsel_cases as cc
import pymf_amd
from conftest import close, load_golden, rel_fro
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN_CASES = ["laesa_29x300_k6_l2", "laesa_29x300_k6_l1", "laesa_29x300_k6_cosine", "laesa_29x300_k6_origin",
                "gmap_29x300_k6_pca", "gmap_29x300_k6_aa", "gmap_29x300_k6_nmf"]


def model(name, V=None):
    c = cc.case(name)
    V = c["V"] if V is None else V
    if c["rule"] == "laesa":
        return c, pymf_amd.LAESA(V, num_bases=c["k"], dist_measure=c["what"], init=c["init"])
    return c, pymf_amd.GMAP(V, num_bases=c["k"], method=c["what"], robust_map=False)


def device(name, **kw):
    c, mdl = model(name)
    mdl.factorize(**kw)
    return c, mdl


def check_select_and_w(name, c, mdl):
    print("%s select %s" % (name, mdl.select))
    assert mdl.select == c["select"]
    assert all(type(s) is int for s in mdl.select)
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float32), c["V"][:, c["select"]])


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_parity(name):
    c, mdl = device(name)
    check_select_and_w(name, c, mdl)
    H = np.asarray(mdl.H)
    assert H.dtype == np.float64 and H.shape == c["H"].shape
    dh = rel_fro(H, c["H"], name + " H")
    df = abs(mdl.ferr[0] - c["ferr"]) / c["ferr"]
    print("%s H deviation %.3e (tol %.3e)  ferr deviation %.3e (tol %.3e)  min H %.3e  max |sum - 1| %.3e" % (
        name, float(dh), cc.H_TOL, df, cc.FERR_TOL, H.min(), np.abs(H.sum(axis=0) - 1.0).max()))
    assert dh <= cc.H_TOL
    close(mdl.ferr[0], c["ferr"], rtol=cc.FERR_TOL, what=name + " ferr")
    assert H.min() >= 0.0
    assert np.abs(H.sum(axis=0) - 1.0).max() <= 1e-5


@pytest.mark.parametrize("name", sorted(cc.PANEL_CASES))
def test_panel_ranges_select_and_w(name):
    """Several panels per workgroup and the second trip of the quad loop: selection and W only (colsel_cases.py)."""
    c, mdl = device(name, compute_h=False, compute_err=False)
    check_select_and_w(name, c, mdl)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_parity(name):
    """The same cases against what the reference itself wrote (tests/golden/gen_golden_colsel.py)."""
    g = load_golden(name)
    c, mdl = device(name)
    assert mdl.select == [int(s) for s in g["select"]]
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float64), g["W"])
    assert rel_fro(mdl.H, g["H"], name + " golden H") <= cc.H_TOL
    close(mdl.ferr[0], g["ferr"][0], rtol=cc.FERR_TOL, what=name + " golden ferr")


@pytest.mark.parametrize("name", ["laesa_doc_2x3_k2", "gmap_doc_2x3_k2", "gmap_37x29_k5"])
def test_small_goldens(name):
    g = load_golden(name)
    cls = pymf_amd.LAESA if name.startswith("laesa") else pymf_amd.GMAP
    kw = {} if name.startswith("laesa") else {"robust_map": False}
    mdl = cls(g["V"], num_bases=int(g["k"]), **kw)
    mdl.factorize()
    assert mdl.select == [int(s) for s in g["select"]]
    assert np.array_equal(np.asarray(mdl.W, dtype=np.float64), g["W"])
    close(mdl.H, g["H"], rtol=0, atol=1e-6, what=name + " H")
    assert abs(mdl.ferr[0] - g["ferr"][0]) <= 1e-6 * max(1.0, g["ferr"][0])


@pytest.mark.parametrize("name", ["laesa_doc_userw", "gmap_doc_userw"])
def test_user_w_matches_golden(name):
    g = load_golden(name)
    mdl = pymf_amd.LAESA(g["V"], num_bases=2) if name.startswith("laesa") else pymf_amd.GMAP(g["V"], num_bases=2, robust_map=False)
    mdl.W = g["W"].copy()
    mdl.factorize(compute_w=False)
    assert np.array_equal(mdl.W, g["W"])
    close(mdl.H, g["H"], rtol=0, atol=1e-6, what=name + " H")
    assert abs(mdl.ferr[0] - g["ferr"][0]) <= 1e-6


@pytest.mark.parametrize("name", ["laesa_29x300_k6_l2", "gmap_29x300_k6_pca"])
def test_hooks_by_hand_equal_factorize(name):
    c, ref = device(name)
    _, mdl = model(name)
    mdl.update_w()
    mdl.update_h()
    assert mdl.select == ref.select
    assert np.array_equal(mdl.W, ref.W)
    assert np.array_equal(mdl.H, ref.H)
    assert mdl.frobenius_norm() == ref.ferr[0]


@pytest.mark.parametrize("name", ["laesa_64x4113_k8", "gmap_64x4113_k8"])
def test_second_factorize_same_bits(name):
    c, mdl = device(name)
    sel, W, H, ferr = list(mdl.select), np.array(mdl.W), np.array(mdl.H), mdl.ferr[0]
    mdl.factorize()
    assert mdl.select == sel
    assert np.array_equal(mdl.W, W) and np.array_equal(mdl.H, H) and mdl.ferr[0] == ferr


def context(name, rule, what=0, init=0):
    c = cc.case(name)
    ctx = _lib.Context(_lib.ALGO_SIVM, c["V"].shape[0], c["V"].shape[1], c["k"])
    ctx.set_v_dense(c["V"])
    ctx.set_option("sivm_rule", rule)
    if rule == 2:
        ctx.set_option("gmap_method", what)
    else:
        ctx.set_option("sivm_metric", what)
        ctx.set_option("sivm_init", init)
    return c, ctx


def test_sivm_select_keeps_sivms_rule():
    """pmf_sivm_select on a context under sivm_rule = 1 answers as on a plain SIVM context (SIVM_CUR depends on it), and does
    not disturb the context's own LAESA selection."""
    import sivm_cases as sc
    s = sc.case("29x300_k6_origin")                            # (on the 'fastmap' cases the two rules select alike)
    c, ctx = context("laesa_29x300_k6_origin", 1, 0, 1)
    try:
        assert np.array_equal(c["V"], s["V"])
        assert s["select"] != c["select"]                      # the two rules differ on these data
        ctx.update_w()
        assert ctx.get_select().tolist() == c["select"]
        assert ctx.sivm_select(s["k"], False, 0, 1, path=1).tolist() == s["select"]
        assert ctx.get_select().tolist() == c["select"]
    finally:
        ctx.close()


@pytest.mark.parametrize("name,rule,what,init,kernel,launches", [
    ("laesa_29x300_k6_l2", 1, 0, 0, "k_laesa_pass<l2>", 8),
    ("laesa_29x300_k6_l1", 1, 1, 0, "k_laesa_pass<l1>", 8),
    ("laesa_29x300_k6_cosine", 1, 2, 0, "k_laesa_pass<cosine>", 8),
    ("laesa_29x300_k6_origin", 1, 0, 1, "k_laesa_pass<l2>", 6),
    ("gmap_29x300_k6_pca", 2, 0, 0, "k_gmap_pass<pca>", 6),
    ("gmap_29x300_k6_aa", 2, 1, 0, "k_gmap_pass<aa>", 6),
    ("gmap_29x300_k6_nmf", 2, 2, 0, "k_gmap_pass<nmf>", 6),
])
def test_launch_counts(name, rule, what, init, kernel, launches):
    """k + 2 ('fastmap') or k ('origin') launches of k_laesa_pass, k of k_gmap_pass, through the profile interface; the site of
    k_sivm_pass sees none of them."""
    c, ctx = context(name, rule, what, init)
    try:
        ctx.profile_enable(True)
        ctx.update_w()
        stats = ctx.kernel_stats()
        print(name, stats["name"], stats["launches"])
        assert ctx.get_select().tolist() == c["select"]
        assert stats["name"] == kernel and stats["launches"] == launches
        m, np_ = c["V"].shape[0], -(-c["V"].shape[1] // 64) * 64
        assert stats["bytes_per_launch"] == 4.0 * m * np_ + (16.0 if rule == 1 else 24.0) * np_
        ctx.set_option("sivm_rule", 0)                         # back to SIVM's rule: its site starts from zero
        assert ctx.kernel_stats()["name"].startswith("k_sivm_pass<") and ctx.kernel_stats()["launches"] == 0
        ctx.profile_enable(False)
    finally:
        ctx.close()


def test_option_refusals():
    ctx = _lib.Context(_lib.ALGO_NMF, 64, 64, 4)
    try:
        for name in ("sivm_rule", "gmap_method"):
            with pytest.raises(_lib.PmfError, match="SIVM contexts only"):
                ctx.set_option(name, 1)
    finally:
        ctx.close()
    ctx = _lib.Context(_lib.ALGO_SIVM, 8, 64, 2)
    try:
        for name, text in (("sivm_rule", "0 \\(SIVM\\), 1 \\(LAESA\\) or 2 \\(GMAP\\)"), ("gmap_method", "0 \\(pca\\), 1 \\(aa\\) or 2 \\(nmf\\)")):
            for value in (-1, 3):
                with pytest.raises(_lib.PmfError, match=text):
                    ctx.set_option(name, value)
            for value in (2, 1, 0):
                ctx.set_option(name, value)
    finally:
        ctx.close()
