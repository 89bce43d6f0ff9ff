"""pymf_amd.CURSL on the MI355X against the reference goldens and the float64 oracle (tests/cursl_oracle.py) on the cases of
tests/cursl_cases.py, each run under the golden's seed.  The draws must equal the golden's exactly; the cumulative
probabilities the oracle's within tol_cum = 1e-9 x (1 + lambda_kk / (lambda_kk - lambda_kk+1)) (1e-9: what tests/test_gpu_svd.py
holds the float64 Jacobi results to; the factor: what the gap at the cut makes of it -- tests/test_cursl_cases.py keeps every
draw 100 tol_cum away from every cumulative sum); each unnormalised leverage vector sums to its kk within 1e-9 kk (the rows of
V are orthonormal: no oracle needed); C, R, the middle factor and the error as tests/test_gpu_cur.py holds CMD's."""
import json
import os
import warnings

import numpy as np
import pytest

import cur_cases as cc
import cursl_cases as csc
import cursl_oracle as cso
import pymf_amd
from conftest import LEDGER_PATH, Measured, load_golden
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = sorted(csc.CURSL_CASES)
SUM_RTOL = 1e-9

_parity = {}


def measured(value, what):
    m = Measured(value)
    m.what = what
    _parity[what] = float(value)
    return m


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    if not _parity:                                           # nothing ran (no device): an earlier record stays
        return
    try:
        out = os.path.dirname(LEDGER_PATH)                    # beside the session's ledger; committed as profiles/cursl_parity.json
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "cursl_parity.json"), "w") as f:
            json.dump({"achieved": _parity}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


_runs = {}


def factorize(name):
    c = csc.case(name)
    mdl = pymf_amd.CURSL(c["data"], rrank=c["rrank"])
    np.random.seed(c["seed"])
    mdl.factorize()
    return mdl


def device_run(name):
    if name not in _runs:
        _runs[name] = factorize(name)
    return csc.case(name), _runs[name]


def one_ulp(got, want):
    return bool(np.all(np.abs(got - want) <= np.spacing(np.abs(want))))


def cum_dev(lev, k, p_oracle):
    p = lev / k
    p = p / p.sum()
    return float(np.max(np.abs(np.cumsum(p) - np.cumsum(p_oracle.ravel()))))


@pytest.mark.parametrize("name", NAMES)
def test_parity(name):
    c, mdl = device_run(name)
    g = load_golden("cursl_" + name)
    tag = "cursl %s " % name
    d64 = c["data"].astype(np.float64)
    # sampling
    for q in ("_rid", "_cid", "_rcnt", "_ccnt"):
        assert np.array_equal(np.asarray(getattr(mdl, q), dtype=np.float64), g[q[1:]].astype(np.float64)), q
    assert (mdl._crank, mdl._rrank) == (c["k_rows"], c["k_cols"])
    lev_r, lev_c = mdl._context().cur_leverage(mdl._crank, mdl._rrank)
    dr, dc = cum_dev(lev_r, mdl._crank, c["prow"]), cum_dev(lev_c, mdl._rrank, c["pcol"])
    gr, gc = cum_dev(lev_r, mdl._crank, g["prow"]), cum_dev(lev_c, mdl._rrank, g["pcol"])
    sr, sc = abs(lev_r.sum() - c["kk_r"]) / c["kk_r"], abs(lev_c.sum() - c["kk_c"]) / c["kk_c"]
    assert np.all(lev_r >= 0.0) and np.all(lev_c >= 0.0)
    # factors
    assert mdl.U is mdl._C and mdl.S is mdl._U and mdl.V is mdl._R
    assert mdl.U.dtype == mdl.S.dtype == mdl.V.dtype == np.float64
    assert mdl.U.shape == c["C"].shape and mdl.S.shape == c["U"].shape and mdl.V.shape == c["R"].shape
    assert one_ulp(mdl.U, d64[:, c["cid"]] * np.sqrt(c["ccnt"])) and one_ulp(mdl.V, np.sqrt(c["rcnt"])[:, None] * d64[c["rid"], :])
    du, dg = cc.rel_max(mdl.S, c["U"]), cc.rel_max(mdl.S, g["U"])
    dfn = abs(mdl.frobenius_norm() - c["ferr"]) / np.linalg.norm(d64)
    dfg = abs(mdl.frobenius_norm() - float(g["ferr"])) / np.linalg.norm(d64)
    print("%scumulative rows %.3e cols %.3e golden %.3e %.3e (tol_cum %.3e)  sums %.3e %.3e (tol %.1e)  U %.3e golden %.3e (tol_U %.3e)  "
          "frobenius_norm %.3e golden %.3e (tol %.3e)" % (tag, dr, dc, gr, gc, c["tol_cum"], sr, sc, SUM_RTOL, du, dg, c["tol_U"], dfn, dfg,
                                                          csc.device_tol_ferr()))
    assert measured(dr, tag + "cumulative prow") <= c["tol_cum"]
    assert measured(dc, tag + "cumulative pcol") <= c["tol_cum"]
    assert measured(gr, tag + "cumulative prow golden") <= c["tol_cum"]
    assert measured(gc, tag + "cumulative pcol golden") <= c["tol_cum"]
    assert measured(sr, tag + "row leverage sum") <= SUM_RTOL
    assert measured(sc, tag + "column leverage sum") <= SUM_RTOL
    assert measured(du, tag + "U") <= c["tol_U"]
    assert measured(dg, tag + "U golden") <= c["tol_U"]
    assert measured(dfn, tag + "frobenius_norm") <= csc.device_tol_ferr()
    assert measured(dfg, tag + "frobenius_norm golden") <= csc.device_tol_ferr()


@pytest.mark.parametrize("name", ["130x2100", "2100x130"])
def test_two_runs_same_bits(name):
    c, mdl = device_run(name)
    again = factorize(name)
    assert np.array_equal(again.U, mdl.U) and np.array_equal(again.S, mdl.S) and np.array_equal(again.V, mdl.V)
    assert again.frobenius_norm() == mdl.frobenius_norm()
    l1, l2 = mdl._context().cur_leverage(mdl._crank, mdl._rrank), again._context().cur_leverage(mdl._crank, mdl._rrank)
    assert np.array_equal(l1[0], l2[0]) and np.array_equal(l1[1], l2[1])
    U, S, V = mdl.U, mdl.S, mdl.V
    np.random.seed(c["seed"])
    mdl.factorize()                                            # the same object, the same context
    assert np.array_equal(mdl.U, U) and np.array_equal(mdl.S, S) and np.array_equal(mdl.V, V)
    l3 = mdl._context().cur_leverage(mdl._crank, mdl._rrank)
    assert np.array_equal(l1[0], l3[0]) and np.array_equal(l1[1], l3[1])


def code_of(call):
    with pytest.raises(_lib.PmfError) as ei:
        call()
    return ei.value.code


def test_cabi_alone():
    c = csc.case("37x29")
    m, n = c["data"].shape
    ctx = _lib.Context(_lib.ALGO_CUR, m, n, 5)
    ctx.set_v_dense(c["data"])
    row, col = ctx.cur_leverage(5, 5)
    assert row.shape == (m,) and col.shape == (n,)
    assert cum_dev(row, 5, c["prow"]) <= c["tol_cum"] and cum_dev(col, 5, c["pcol"]) <= c["tol_cum"]
    # NULL for either output
    r_only, none = ctx.cur_leverage(5, 5, want="r")
    assert none is None and np.array_equal(r_only, row)
    none, c_only = ctx.cur_leverage(5, 5, want="c")
    assert none is None and np.array_equal(c_only, col)
    # the two ranks are independent: rows with 3 vectors, columns with 5
    r3, c5 = ctx.cur_leverage(3, 5)
    assert np.array_equal(c5, col) and abs(r3.sum() - 3.0) <= 3 * SUM_RTOL and np.all(r3 <= row + 1e-12)
    # refusals
    assert code_of(lambda: ctx.cur_leverage(0, 5)) == _lib.PMF_EINVAL
    assert code_of(lambda: ctx.cur_leverage(5, 0)) == _lib.PMF_EINVAL
    big = csc.case("200x200")
    wide = _lib.Context(_lib.ALGO_CUR, 200, 200, 128)
    wide.set_v_dense(big["data"])
    assert code_of(lambda: wide.cur_leverage(200, 128)) == _lib.PMF_EINVAL      # min(k, rank) = 200 > 128
    assert abs(wide.cur_leverage(200, 128, want="c")[1].sum() - 128.0) <= 128 * SUM_RTOL   # (the side that is not asked for is not checked)
    wide.close()
    nmf = _lib.Context(_lib.ALGO_NMF, m, n, 5)
    nmf.set_v_dense(c["data"])
    assert code_of(lambda: nmf.cur_leverage(5, 5)) == _lib.PMF_EINVAL           # CUR / CMD contexts only
    nmf.close()
    # other data: other leverages (the cached eigenpairs go with the data)
    other = csc.spectrum_data(m, n, 5, 171)
    ctx.set_v_dense(other)
    row2, col2 = ctx.cur_leverage(5, 5)
    want_r, _, _ = cso.leverage(other.astype(np.float64).T, 5)
    want_c, _, _ = cso.leverage(other.astype(np.float64), 5)
    assert not np.array_equal(row2, row) and not np.array_equal(col2, col)
    assert np.max(np.abs(row2 - want_r)) <= 1e-7 and np.max(np.abs(col2 - want_c)) <= 1e-7
    ctx.close()


@pytest.mark.parametrize("name", ["37x29", "29x300"])
def test_leverage_and_greedy_select_share_the_eigenpairs(name):
    """pmf_greedy_select and pmf_cur_leverage on one context, in either order, against contexts of their own: the same bits."""
    c = csc.case(name)
    m, n = c["data"].shape

    def fresh():
        ctx = _lib.Context(_lib.ALGO_CUR, m, n, 5)
        ctx.set_v_dense(c["data"])
        return ctx
    a, b = fresh(), fresh()
    lev = a.cur_leverage(5, 5)
    sel = [b.greedy_select(4, transposed=t) for t in (False, True)]
    a.close()
    b.close()
    first, second = fresh(), fresh()
    lev1 = first.cur_leverage(5, 5)
    sel1 = [first.greedy_select(4, transposed=t) for t in (False, True)]
    sel2 = [second.greedy_select(4, transposed=t) for t in (False, True)]
    lev2 = second.cur_leverage(5, 5)
    first.close()
    second.close()
    for got in (lev1, lev2):
        assert np.array_equal(got[0], lev[0]) and np.array_equal(got[1], lev[1])
    for got in (sel1, sel2):
        assert np.array_equal(got[0], sel[0]) and np.array_equal(got[1], sel[1])


def test_profile_cur_chooses_the_timed_launch():
    """pmf_set_option "profile_cur": 0 the cross product of pmf_cur_compute, 1 k_lev_f64 (named and counted per call), 2 k_cur_sqnorms."""
    c = csc.case("37x29")
    m, n = c["data"].shape
    nmf = _lib.Context(_lib.ALGO_NMF, m, n, 5)
    assert code_of(lambda: nmf.set_option("profile_cur", 1)) == _lib.PMF_EINVAL     # CUR / CMD contexts only
    nmf.close()
    ctx = _lib.Context(_lib.ALGO_CUR, m, n, 5)
    ctx.set_v_dense(c["data"])
    assert code_of(lambda: ctx.set_option("profile_cur", 3)) == _lib.PMF_EINVAL
    assert code_of(lambda: ctx.set_option("profile_cur", -1)) == _lib.PMF_EINVAL
    plain = ctx.cur_leverage(5, 3)
    ctx.set_option("profile_cur", 1)
    ctx.profile_enable(True)
    timed = ctx.cur_leverage(5, 3)                             # tall data: the rows are the long side, five vectors, one operand tile
    st = ctx.kernel_stats()
    assert st["name"] == "k_lev_f64<false,1>" and st["launches"] == 1 and st["mean_ms"] > 0.0
    assert st["flops_per_launch"] == 2.0 * m * n * 5 and st["bytes_per_launch"] == 4.0 * 64 * 64 + 8.0 * 64
    assert np.array_equal(timed[0], plain[0]) and np.array_equal(timed[1], plain[1])
    ctx.profile_enable(True)
    ctx.cur_leverage(5, 3, want="c")                           # the eigenvector side alone: no pass over the data
    assert ctx.kernel_stats()["launches"] == 0
    ctx.set_option("profile_cur", 2)
    ctx.profile_enable(True)
    ctx.cur_sqnorms()
    st = ctx.kernel_stats()
    assert st["name"] == "k_cur_sqnorms" and st["launches"] == 1 and st["mean_ms"] > 0.0
    ctx.set_option("profile_cur", 0)
    ctx.profile_enable(True)
    ctx.cur_leverage(5, 3)
    ctx.cur_sqnorms()
    st = ctx.kernel_stats()
    assert st["name"] == "k_prod_f64<true,full>" and st["launches"] == 0
    ctx.cur_compute(c["rid"], c["rcnt"], c["cid"], c["ccnt"])
    assert ctx.kernel_stats()["launches"] >= 1
    ctx.profile_enable(False)
    ctx.close()


def test_rrank_zero_takes_all_rows_and_columns():
    """rrank = 0 on cursl.py's example: the rows are sampled with k = _crank = 3, the columns with k = _rrank = 2 (both beyond
    nothing but the rank, 2)."""
    c = csc.case("doc_2x3")
    mdl = pymf_amd.CURSL(c["data"])
    assert (mdl._rrank, mdl._crank) == (2, 3)
    prow, pcol = mdl.sample_probability()
    want_r, want_c = cso.sample_probability(c["data"].astype(np.float64), 2, 3)
    assert prow.shape == (2, 1) and pcol.shape == (3, 1)
    assert np.max(np.abs(prow - want_r)) <= 1e-9 and np.max(np.abs(pcol - want_c)) <= 1e-9
    assert abs(prow.sum() - 1.0) <= 1e-15 and abs(pcol.sum() - 1.0) <= 1e-15
    np.random.seed(c["seed"])
    mdl.factorize()
    rid, cid, rcnt, ccnt, _, _ = cso.draw(c["data"].astype(np.float64), 0, c["seed"])
    assert np.array_equal(mdl._rid, rid) and np.array_equal(mdl._cid, cid)
    assert np.array_equal(mdl._rcnt, rcnt) and np.array_equal(mdl._ccnt, ccnt) and rcnt.sum() == 2 and ccnt.sum() == 3


def test_float64_data_warns_once():
    c = csc.case("37x29")
    mdl = pymf_amd.CURSL(c["data"].astype(np.float64), rrank=5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        np.random.seed(c["seed"])
        mdl.factorize()
        mdl.factorize()
    assert len([x for x in w if issubclass(x.category, pymf_amd.nmf.PrecisionWarning)]) == 1
