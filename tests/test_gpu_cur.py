"""pymf_amd.CUR / CMD / pinv on the MI355X against the reference goldens and the float64 oracle (tests/cur_oracle.py) on the
cases of tests/cur_cases.py, each run under the golden's seed.  The draws must equal the golden's exactly; C and R the data's
rows and columns times sqrt(count) to 1 ulp; the middle factor within tol_U = (kappa_C + kappa_R) x 1e-9 of max |U| (the
Gram matrices and the middle product are float64: only Jacobi's convergence, which tests/test_gpu_svd.py holds to 1e-9, and
its amplification by the pseudo-inverses stand between them); the error within 4 x the deviation of the oracle's float32 twin
(tests/golden/cur_tolerances.json)."""
import json
import os
import warnings

import numpy as np
import pytest

import cur_cases as cc
import cur_oracle as co
import pymf_amd
import svd_cases as sc
from conftest import LEDGER_PATH, Measured, load_golden
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

CLASSES = {"cur": pymf_amd.CUR, "cmd": pymf_amd.CMD}
PAIRS = [(name, kind) for name in sorted(cc.CUR_CASES) for kind in cc.KINDS]
SQNORM_RTOL = 1e-13          # sums of exact products in float64 on either side: only the order differs
S_RTOL = 1e-9                # tests/test_gpu_svd.py: the singular values against numpy.linalg.svd

_parity = {}


def measured(value, what):
    m = Measured(value)
    m.what = what
    _parity[what] = float(value)
    return m


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    try:
        out = os.path.dirname(LEDGER_PATH)                    # beside the session's ledger; committed as profiles/cur_parity.json
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "cur_parity.json"), "w") as f:
            json.dump({"achieved": _parity}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


_runs = {}


def factorize(name, kind):
    c = cc.case(name, kind)
    mdl = CLASSES[kind](c["data"], rrank=c["rrank"])
    np.random.seed(c["seed"])
    mdl.factorize()
    return mdl


def device_run(name, kind):
    if (name, kind) not in _runs:
        _runs[(name, kind)] = factorize(name, kind)
    return cc.case(name, kind), _runs[(name, kind)]


def one_ulp(got, want):
    return bool(np.all(np.abs(got - want) <= np.spacing(np.abs(want))))


@pytest.mark.parametrize("name,kind", PAIRS)
def test_parity(name, kind):
    c, mdl = device_run(name, kind)
    g = load_golden("%s_%s" % (kind, name))
    tag = "%s %s " % (kind, name)
    d64 = c["data"].astype(np.float64)
    # sampling
    for q in ("_rid", "_cid", "_rcnt", "_ccnt"):
        assert np.array_equal(np.asarray(getattr(mdl, q), dtype=np.float64), g[q[1:]].astype(np.float64)), q
    row_sq, col_sq = mdl._context().cur_sqnorms()
    sq = d64 ** 2
    dn = max(float(np.max(np.abs(row_sq - sq.sum(axis=1)) / sq.sum(axis=1))), float(np.max(np.abs(col_sq - sq.sum(axis=0)) / sq.sum(axis=0))))
    # factors
    assert mdl.U is mdl._C and mdl.S is mdl._U and mdl.V is mdl._R
    assert mdl.U.dtype == mdl.S.dtype == mdl.V.dtype == np.float64
    assert mdl.U.shape == c["C"].shape and mdl.S.shape == c["U"].shape and mdl.V.shape == c["R"].shape
    assert one_ulp(mdl.U, d64[:, c["cid"]] * np.sqrt(c["ccnt"])) and one_ulp(mdl.V, np.sqrt(c["rcnt"])[:, None] * d64[c["rid"], :])
    # middle factor
    du, dg = cc.rel_max(mdl.S, c["U"]), cc.rel_max(mdl.S, g["U"])
    # error
    dfn = abs(mdl.frobenius_norm() - c["ferr"]) / np.linalg.norm(d64)
    dfg = abs(mdl.frobenius_norm() - float(g["ferr"])) / np.linalg.norm(d64)
    print("%snorms %.3e (tol %.1e)  U %.3e golden %.3e (tol_U %.3e)  frobenius_norm %.3e golden %.3e (tol %.3e)" % (
        tag, dn, SQNORM_RTOL, du, dg, c["tol_U"], dfn, dfg, cc.device_tol_ferr()))
    assert measured(dn, tag + "sqnorms") <= SQNORM_RTOL
    assert measured(du, tag + "U") <= c["tol_U"]
    assert measured(dg, tag + "U golden") <= c["tol_U"]
    assert measured(dfn, tag + "frobenius_norm") <= cc.device_tol_ferr()
    assert measured(dfg, tag + "frobenius_norm golden") <= cc.device_tol_ferr()


@pytest.mark.parametrize("name", ["130x2100", "2100x130"])
def test_two_runs_same_bits(name):
    for kind in cc.KINDS:
        c, mdl = device_run(name, kind)
        again = factorize(name, kind)
        assert np.array_equal(again.U, mdl.U) and np.array_equal(again.S, mdl.S) and np.array_equal(again.V, mdl.V)
        assert again.frobenius_norm() == mdl.frobenius_norm()
        U, S, V = mdl.U, mdl.S, mdl.V
        np.random.seed(c["seed"])
        mdl.factorize()                                        # the same object, the same context
        assert np.array_equal(mdl.U, U) and np.array_equal(mdl.S, S) and np.array_equal(mdl.V, V)
        p1, p2 = mdl._context().cur_sqnorms(), again._context().cur_sqnorms()
        assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])


@pytest.mark.parametrize("name", ["29x300", "2100x130"])
def test_compute_ucr_with_indices_set_by_hand(name):
    """computeUCR() alone: unsorted indices, a repeated one, one index of -1, counts above 1."""
    data = cc.data(name)
    d64 = data.astype(np.float64)
    rows, cols = data.shape
    rid, rcnt = np.array([7, -1, 3, 7]), np.array([1.0, 2.0, 1.0, 1.0])
    cid, ccnt = np.array([cols // 2, 2, -1, 17, 5]), np.array([1.0, 1.0, 3.0, 1.0, 2.0])
    rid_pos, cid_pos = np.where(rid < 0, rid + rows, rid), np.where(cid < 0, cid + cols, cid)
    C, U, R = co.compute_ucr(d64, rid_pos, rcnt, cid_pos, ccnt)
    gram = co.gram_form(d64, rid_pos, rcnt, cid_pos, ccnt)
    assert min(gram["kept_c"].min(), gram["kept_r"].min()) >= 1e-3
    assert max(np.abs(gram["dropped_c"]).max(initial=0.0), np.abs(gram["dropped_r"]).max(initial=0.0)) <= 1e-10
    assert gram["dropped_r"].size == 1                         # the repeated row: a null eigenvalue that must go
    tol_u = (cc.cond(gram["kept_c"]) + cc.cond(gram["kept_r"])) * cc.JACOBI_RTOL
    mdl = pymf_amd.CUR(data, rrank=4)
    mdl._rid, mdl._rcnt, mdl._cid, mdl._ccnt = rid, rcnt, cid, ccnt
    mdl.computeUCR()
    assert mdl.S.shape == (5, 4) and one_ulp(mdl.U, C) and one_ulp(mdl.V, R)
    du = cc.rel_max(mdl.S, U)
    dfn = abs(mdl.frobenius_norm() - co.ferr(d64, C, U, R)) / np.linalg.norm(d64)
    print("%s by hand: U %.3e (tol %.3e) frobenius_norm %.3e (tol %.3e)" % (name, du, tol_u, dfn, cc.device_tol_ferr()))
    assert measured(du, name + " by hand U") <= tol_u
    assert measured(dfn, name + " by hand frobenius_norm") <= cc.device_tol_ferr()
    # a rebound factor is taken from the arrays at hand (SVD.frobenius_norm)
    mdl.S = np.zeros_like(mdl.S)
    assert abs(mdl.frobenius_norm() - np.linalg.norm(d64)) <= 1e-6 * np.linalg.norm(d64)


@pytest.mark.parametrize("name", ["20x30", "300x40"])
def test_pinv(name):
    g = load_golden("pinv_" + name)
    rows, cols = (int(x) for x in g["A_shape"])
    A = np.random.RandomState(int(g["A_seed"])).rand(rows, cols).astype(np.float32)
    P = pymf_amd.pinv(A)
    assert P.shape == (cols, rows) and P.dtype == np.float64
    # pinv = sum_i v_i u_i^T / s_i of SVD's factors: unit vectors within device_tol("U") and device_tol("V"), s_i within S_RTOL
    s = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    bound = (sc.device_tol("U") + sc.device_tol("V") + S_RTOL) * float(np.sum(1.0 / s))
    dg = float(np.max(np.abs(P - g["P"])))
    dn = float(np.max(np.abs(P - np.linalg.pinv(A.astype(np.float64)))))
    print("pinv %s: golden %.3e numpy %.3e (bound %.3e)" % (name, dg, dn, bound))
    assert measured(dg, "pinv %s golden" % name) <= bound
    assert measured(dn, "pinv %s numpy" % name) <= bound


def test_float64_data_warns_once():
    c = cc.case("37x29", "cur")
    mdl = pymf_amd.CUR(c["data"].astype(np.float64), rrank=5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        np.random.seed(c["seed"])
        mdl.factorize()
        mdl.factorize()
    assert len([x for x in w if issubclass(x.category, pymf_amd.nmf.PrecisionWarning)]) == 1


def test_cabi_alone():
    c = cc.case("37x29", "cmd")
    m, n = c["data"].shape
    ctx = _lib.Context(_lib.ALGO_CUR, m, n, 5)
    ctx.set_v_dense(c["data"])
    ctx._cur_shape = (1, 1)
    with pytest.raises(_lib.PmfError):
        ctx.cur_get()                                          # nothing decomposed yet
    for bad in (dict(rid=[0, m], rcnt=[1, 1]), dict(rid=[0, -m - 1], rcnt=[1, 1]), dict(rid=[0, 1], rcnt=[1, 0]),
                dict(rid=list(range(6)), rcnt=[1] * 6)):
        with pytest.raises(_lib.PmfError) as ei:
            ctx.cur_compute(bad["rid"], bad["rcnt"], [0, 1], [1, 1])
        assert ei.value.code == _lib.PMF_EINVAL
    for call in (ctx.update_w, ctx.update_h, lambda: ctx.factorize(1)):
        with pytest.raises(_lib.PmfError) as ei:
            call()
        assert ei.value.code == _lib.PMF_EINVAL
    ctx.cur_compute(c["rid"], c["rcnt"], c["cid"], c["ccnt"])
    C, U, R = ctx.cur_get()
    assert cc.rel_max(U, c["U"]) <= c["tol_U"] and one_ulp(C, c["C"]) and one_ulp(R, c["R"])
    assert ctx.cur_get(want="U")[0] is None and ctx.cur_get(want="U")[2] is None
    assert abs(ctx.frobenius() - c["ferr"]) <= cc.device_tol_ferr() * np.linalg.norm(c["data"].astype(np.float64))
    assert ctx.path_name == "cur_cross_f64"
    ctx.set_v_dense(c["data"])                                 # new data: the decomposition is gone
    with pytest.raises(_lib.PmfError):
        ctx.cur_get()
    ctx.close()
