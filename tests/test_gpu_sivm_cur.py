"""pymf_amd.SIVM_CUR on the device against the float64 oracle on the cases of tests/sivm_cur_cases.py and against goldens of the
real reference; pmf_sivm_select's forced paths, its determinism and its refusals.

Device tolerances: 4 x the worst oracle-vs-twin deviation of U and of the error (sivm_cur_cases.TWIN_U_DEV, TWIN_FERR_DEV)."""
import os

import numpy as np
import pytest

import sivm_cur_cases as cc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METRIC = {"l2": 0, "l1": 1, "cosine": 2}
INIT = {"fastmap": 0, "origin": 1}


@pytest.fixture(scope="module")
def pm():
    import pymf_amd
    return pymf_amd


def run(pm, name):
    c = cc.case(name)
    mdl = pm.SIVM_CUR(c["data"], rrank=c["rrank"], dist_measure=c["metric"], init=c["init"])
    mdl.factorize()
    return c, mdl


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_matches_the_oracle(pm, name):
    c, mdl = run(pm, name)
    nrm = np.linalg.norm(c["data"].astype(np.float64))
    print(name, mdl._rid, mdl._cid, "U", cc.rel_max(mdl.S, c["U"]), "tol", cc.device_tol_u(), "ferr", abs(mdl.frobenius_norm() - c["ferr"]) / nrm,
          "tol", cc.device_tol_ferr())
    assert mdl._rid == c["rid"] and mdl._cid == c["cid"]
    assert all(type(s) is int for s in mdl._rid + mdl._cid)
    assert np.array_equal(mdl._rcnt, np.ones(c["rrank"])) and np.array_equal(mdl._ccnt, np.ones(c["rrank"]))
    assert np.array_equal(mdl.U, c["data"][:, c["cid"]].astype(np.float64))
    assert np.array_equal(mdl.V, c["data"][c["rid"], :].astype(np.float64))
    assert mdl.S.shape == c["U"].shape and cc.rel_max(mdl.S, c["U"]) <= cc.device_tol_u()
    assert abs(mdl.frobenius_norm() - c["ferr"]) <= cc.device_tol_ferr() * nrm


@pytest.mark.parametrize("name", cc.GOLDEN)
def test_golden(pm, name):
    g = np.load(os.path.join(GOLD, "sivmcur_" + name + ".npz"))
    c, mdl = run(pm, name)
    assert mdl._rid == g["rid"].tolist() and mdl._cid == g["cid"].tolist()
    print(name, "U", cc.rel_max(mdl.S, g["U"]))
    assert cc.rel_max(mdl.S, g["U"]) <= cc.device_tol_u()


@pytest.mark.parametrize("name", ["29x300_cosine_fastmap", "300x29"])
@pytest.mark.parametrize("metric,init", [("l2", "origin"), ("cosine", "fastmap")])
def test_forced_paths_agree_and_repeat(pm, name, metric, init):
    """Both kernels, with and without the transposed copy, at small shapes: the column-panel pass (path 1) and the long-sample
    pass (path 2) select what the automatic path and the oracle select, and a second call gives the same array.  The data of
    the two cases serve both measures: every argmax of every combination keeps its gap (asserted here)."""
    from pymf_amd import _lib
    d = cc.case(name)["data"]
    d64 = d.astype(np.float64)
    ctx = _lib.Context(_lib.ALGO_CUR, d.shape[0], d.shape[1], 6)
    try:
        ctx.set_v_dense(d)
        for transposed in (False, True):
            want, scores = cc.all_scores(d64.T if transposed else d64, 6, metric, init)
            assert min(g[0] for g in cc.gaps(scores, want, init)) >= 1e-3
            auto = ctx.sivm_select(6, transposed, METRIC[metric], INIT[init])
            print(name, metric, init, transposed, auto.tolist(), want)
            assert auto.dtype == np.int32 and auto.tolist() == want
            for path in (1, 2):
                a = ctx.sivm_select(6, transposed, METRIC[metric], INIT[init], path=path)
                b = ctx.sivm_select(6, transposed, METRIC[metric], INIT[init], path=path)
                assert np.array_equal(a, auto), (path, a, auto)
                assert np.array_equal(a, b)
    finally:
        ctx.close()


def test_tie_takes_the_lower_index(pm):
    c, mdl = run(pm, cc.TIE_CASE)
    rows, cols, rrank, seed, offset, scale, metric, init = cc.CASES[cc.TIE_CASE]
    src, dup = cc.tie_rows(cc.spectrum_data(rows, cols, seed, offset, scale), rrank, metric, init)
    assert mdl._rid[cc.TIE_ROUND] == src and dup not in mdl._rid and mdl._rid == c["rid"]
    from pymf_amd import _lib
    ctx = _lib.Context(_lib.ALGO_CUR, rows, cols, rrank)
    try:
        ctx.set_v_dense(c["data"])
        for path in (1, 2):                                            # the tie in both kernels
            assert ctx.sivm_select(rrank, True, 0, 1, path=path).tolist() == c["rid"]
    finally:
        ctx.close()


def test_sample_on_a_foreign_matrix_goes_through_sivm(pm):
    c = cc.case("29x300_l2")
    other = cc.case("29x300_fastmap")["data"]
    mdl = pm.SIVM_CUR(c["data"], rrank=6)
    got = mdl.sample(other, 6)
    ref = pm.SIVM(other, num_bases=6, dist_measure="l2", init="origin")
    ref.factorize(compute_h=False, compute_err=False)
    assert got == ref.select and got[0] == -1 and all(type(s) is int for s in got)
    assert mdl.sample(c["data"], 6) == c["cid"] and mdl.sample(c["data"].transpose(), 6) == c["rid"]
    assert mdl.sample(np.ascontiguousarray(c["data"].T), 6) == c["rid"]     # a copy of the transposed data: SIVM's own kernel


def test_data_replaced_in_place_is_noticed(pm):
    c = cc.case("29x300_l2")
    d = c["data"].copy()
    mdl = pm.SIVM_CUR(d, rrank=6)
    mdl.factorize()
    assert mdl._rid == c["rid"] and mdl._cid == c["cid"]
    d[:] = cc.REPLACED_DATA()
    d64 = d.astype(np.float64)
    rid, sr = cc.all_scores(d64.T, 6, "l2", "origin")
    cid, scs = cc.all_scores(d64, 6, "l2", "origin")
    assert min(g[0] for g in cc.gaps(sr, rid, "origin") + cc.gaps(scs, cid, "origin")) >= 1e-3 and (rid, cid) != (c["rid"], c["cid"])
    mdl.factorize()
    assert mdl._rid == rid and mdl._cid == cid
    assert np.array_equal(mdl.U, d64[:, cid]) and np.array_equal(mdl.V, d64[rid, :])


def test_bad_arguments_touch_nothing(pm):
    from pymf_amd import _lib
    d = cc.case("29x300_l2")["data"]
    ctx = _lib.Context(_lib.ALGO_CUR, 29, 300, 6)
    big = _lib.Context(_lib.ALGO_CUR, 8, 16448, 4)                     # 16 448 columns: beyond either kernel's limit on one side
    nmf = _lib.Context(_lib.ALGO_NMF, 29, 300, 6)
    try:
        ctx.set_v_dense(d)
        big.set_v_dense(np.ones((8, 16448), dtype=np.float32))
        nmf.set_v_dense(d)

        def code(cx, transposed, nsel, metric, init, path):
            out = np.full(80, -77, dtype=np.int32)
            rc = cx._lib.pmf_sivm_select(cx._h, transposed, nsel, metric, init, path, out.ctypes.data)
            assert np.all(out == -77) or rc == _lib.PMF_OK
            return rc

        assert code(ctx, 0, 0, 0, 0, 0) == _lib.PMF_EINVAL
        assert code(ctx, 0, 65, 0, 0, 0) == _lib.PMF_EINVAL
        assert code(ctx, 0, 6, 3, 0, 0) == _lib.PMF_EINVAL
        assert code(ctx, 0, 6, 0, 2, 0) == _lib.PMF_EINVAL
        assert code(ctx, 0, 6, 0, 0, 3) == _lib.PMF_EINVAL
        assert code(nmf, 0, 6, 0, 0, 0) == _lib.PMF_EINVAL             # a context of another algorithm
        assert code(big, 0, 4, 0, 1, 2) == _lib.PMF_EINVAL             # 16 448 candidates for the long-sample pass
        assert code(big, 1, 4, 0, 1, 1) == _lib.PMF_EINVAL             # samples of dimension 16 448 for the column-panel pass
        assert code(big, 0, 4, 0, 1, 0) == _lib.PMF_OK and code(big, 1, 4, 0, 1, 0) == _lib.PMF_OK
        assert ctx.sivm_select(6, True, 0, 1).tolist() == cc.case("29x300_l2")["rid"]      # the context still works
    finally:
        ctx.close()
        big.close()
        nmf.close()


def test_limits(pm):
    with pytest.raises(ValueError):
        pm.SIVM_CUR(np.ones((80, 100), dtype=np.float32), rrank=65).factorize()
    with pytest.raises(NotImplementedError):
        pm.SIVM_CUR(np.ones((8, 100), dtype=np.float32), rrank=2, dist_measure="kl").factorize()
