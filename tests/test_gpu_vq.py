"""vq / pdist on the device: every case of tests/vq_cases.py -- the 245 exact shapes with n <= 257, the three deep ones, every
generic case -- through the C ABI alone (pmf_vq_columns, pmf_vq_assign) and through pymf_amd.vq / pymf_amd.pdist, both directions,
both metrics; every C-ABI call twice with identical bits; the C-ABI refusals; vq(mdl, W)
on a fitted SIVM model.  Exact cases are held with array_equal alone, generic cases to EPS = (m + 4) 2^-24 (vq_cases.py).
Achieved errors are written as parity_vq.json next to the session's parity ledger (conftest.LEDGER_PATH) and committed as
profiles/parity_vq.json."""
import json
import os
import warnings

import numpy as np
import pytest

import pymf_amd
import vq_cases as vc
from pymf_amd import _lib
from conftest import LEDGER_PATH

pytestmark = pytest.mark.gpu

MET = {"l2": 0, "l1": 1}
SMALL_MN = sorted({(m, n) for m, n, _ in vc.exact_shapes() if n <= 257})
_FIG = {}


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    yield
    out = os.path.dirname(LEDGER_PATH)                    # beside the session's ledger; committed as profiles/parity_vq.json
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_vq.json"), "w") as f:
        json.dump(_FIG, f, indent=1, sort_keys=True)
        f.write("\n")


def run_abi(ctx, c, k):
    """Both entries twice: (cols idx, cols dist, asg idx, block), the second run asserted bit-identical to the first."""
    first = None
    for _ in range(2):
        ci, cd = ctx.vq_columns(c.Q, MET[k])
        ai, blk = ctx.vq_assign(c.Q, MET[k], want_idx=True, want_dist=True)
        got = (ci.copy(), cd.copy(), ai.copy(), blk.copy())
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                assert a.tobytes() == b.tobytes()
    return first


def check_exact_abi(ctx, c):
    for k in vc.METRICS:
        ci, cd, ai, blk = run_abi(ctx, c, k)
        assert np.array_equal(ci, c.cols[k]), (c.name, k)
        assert np.array_equal(ai, c.asg[k]), (c.name, k)
        assert np.array_equal(c.squared(k, blk), c.D[k]), (c.name, k)
        assert np.array_equal(cd, blk[np.arange(c.nq), ci]), (c.name, k)            # the distance that won is the block's
        if k == "l2":
            _FIG["exact_l2_root_is_correctly_rounded"] = bool(_FIG.get("exact_l2_root_is_correctly_rounded", True)
                                                              and np.array_equal(blk, c.rounded_root()))


@pytest.mark.parametrize("m,n", SMALL_MN)
def test_exact_cases_c_abi(m, n):
    """One context per (m, n), on the family the width allows; every nq of the set against it."""
    V = None
    ctx = None
    for nq in vc.Q_SET:
        c = vc.exact(m, n, nq)
        if ctx is None or not np.array_equal(V, c.V):
            if ctx is not None:
                ctx.close()
            ctx = _lib.Context(_lib.ALGO_SIVM, m, n, 1)
            ctx.set_v_dense(c.V)
            V = c.V
        check_exact_abi(ctx, c)
    ctx.close()


@pytest.mark.parametrize("m,n,nq", vc.DEEP)
def test_deep_exact_cases_c_abi(m, n, nq):
    """More than one panel per workgroup: ties across a wave, a trip and a workgroup's range inside the wide partition."""
    c = vc.exact(m, n, nq)
    ctx = _lib.Context(_lib.ALGO_SIVM, m, n, 1)
    ctx.set_v_dense(c.V)
    check_exact_abi(ctx, c)
    ctx.close()


def check_exact_python(c):
    """vq and pdist of the package, both directions, both metrics: array_equal alone.  Every call makes its own context."""
    for k in vc.METRICS:
        d = pymf_amd.pdist(c.Q, c.V, metric=k)
        assert d.shape == (c.nq, c.n) and np.array_equal(c.squared(k, d), c.D[k]), (c.name, k)
        dt = pymf_amd.pdist(c.V, c.Q, metric=k)
        assert dt.shape == (c.n, c.nq) and np.array_equal(dt, d.T), (c.name, k)
        # vq(A, B) = argmin(pdist(A, B), axis=0), whichever side the library makes the data
        got = pymf_amd.vq(c.V, c.Q, metric=k)
        assert got.dtype == np.intp and np.array_equal(got, c.cols[k]), (c.name, k)
        got = pymf_amd.vq(c.Q, c.V, metric=k)
        assert got.dtype == np.intp and np.array_equal(got, c.asg[k]), (c.name, k)


@pytest.mark.parametrize("m,n", SMALL_MN)
def test_exact_cases_python(m, n):
    """Every exact shape with n <= 257 through pymf_amd.vq / pymf_amd.pdist: every nq of the set at this (m, n)."""
    for nq in vc.Q_SET:
        check_exact_python(vc.exact(m, n, nq))
    c = vc.exact(m, n, 17)
    assert pymf_amd.pdist(c.Q, c.V).tobytes() == pymf_amd.pdist(c.Q, c.V).tobytes()      # a second call, a second context: the same bits


@pytest.mark.parametrize("m,n,nq", vc.DEEP)
def test_deep_exact_cases_python(m, n, nq):
    check_exact_python(vc.exact(m, n, nq))


@pytest.mark.parametrize("algo,k", [("NMF", 4), ("NMFALS", 4), ("SNMF", 4), ("BNMF", 4), ("RNMF", 4), ("CNMF", 4), ("KMEANS", 4),
                                    ("CMEANS", 4), ("SIVM", 4), ("AA", 4), ("PCA", 64), ("CUR", 4), ("GREEDY", 4)])
def test_any_context_with_dense_resident_data(algo, k):
    """The SIVM family, AA (CHNMF's), Kmeans / Cmeans, the NMF family and the rest: whatever the family allocates around V,
    the sweep reads V [mp][np] of that context (448 columns are padded to 512 on an NMF context)."""
    for m, n, nq in ((64, 65, 17), (5, 257, 16)) + (((7, 448, 15),) if algo in ("NMF", "BNMF") else ()):
        if (m, n, nq) in [s for s in vc.exact_shapes()]:
            c = vc.exact(m, n, nq)
        else:
            c = vc.exact_case(m, n, nq, 7)
        ctx = _lib.Context(getattr(_lib, "ALGO_" + algo), m, n, k)
        ctx.set_v_dense(c.V)
        check_exact_abi(ctx, c)
        ctx.close()


@pytest.mark.parametrize("name", sorted(vc.generic_specs()))
def test_generic_cases(name):
    c = vc.generic(name)
    ctx = _lib.Context(_lib.ALGO_SIVM, c.m, c.n, 1)
    ctx.set_v_dense(c.V)
    for k in vc.METRICS:
        ci, cd, ai, blk = run_abi(ctx, c, k)
        err = c.check_dist(k, blk)
        _FIG["%s/%s/dist_err_over_eps" % (name, k)] = err
        _FIG["%s/%s/cols_equal_reference" % (name, k)] = float((ci == np.argmin(c.ref[k], axis=1)).mean())
        _FIG["%s/%s/asg_equal_reference" % (name, k)] = float((ai == np.argmin(c.ref[k], axis=0)).mean())
        print(name, k, "max |d - d_ref| / (eps d_ref) =", err)
        assert err <= 1.0, (name, k, err)
        assert np.array_equal(cd, blk[np.arange(c.nq), ci])
        assert c.check_index(k, "cols", ci), (name, k)
        assert c.check_index(k, "asg", ai), (name, k)
    ctx.close()


@pytest.mark.parametrize("name", sorted(vc.generic_specs()))
def test_generic_cases_python(name):
    """Every generic case through pymf_amd.vq / pymf_amd.pdist, both metrics, both directions, to the same bound."""
    c = vc.generic(name)
    for k in vc.METRICS:
        d = pymf_amd.pdist(c.Q, c.V, metric=k)
        err = c.check_dist(k, d)
        _FIG["%s/%s/python_dist_err_over_eps" % (name, k)] = err
        assert err <= 1.0, (name, k, err)
        assert np.array_equal(pymf_amd.pdist(c.V, c.Q, metric=k), d.T)
        assert c.check_index(k, "cols", pymf_amd.vq(c.V, c.Q, metric=k)), (name, k)
        assert c.check_index(k, "asg", pymf_amd.vq(c.Q, c.V, metric=k)), (name, k)


def test_a_model_without_factors_serves_vq_from_its_data_alone():
    """A freshly constructed NMF (no W, no H yet): only its data go up; the factors stay unset."""
    c = vc.exact(5, 257, 16)
    mdl = pymf_amd.NMF(c.V, num_bases=3)
    assert np.array_equal(pymf_amd.vq(mdl, c.Q), c.cols["l2"])
    assert np.array_equal(pymf_amd.vq(c.Q, mdl, metric="l1"), c.asg["l1"])
    assert not mdl._has("W") and not mdl._has("H")
    mdl.factorize(niter=2)                                                          # ... and the model goes on as usual
    assert np.array_equal(pymf_amd.vq(mdl, c.Q), c.cols["l2"])


def test_float64_input_is_rounded_with_a_warning():
    c = vc.exact(5, 65, 17)
    with pytest.warns(pymf_amd.nmf.PrecisionWarning):
        got = pymf_amd.vq(c.V.astype(np.float64), c.Q.astype(np.float64))
    assert np.array_equal(got, c.cols["l2"])


def test_vq_maps_the_bases_of_a_fitted_sivm_onto_its_selection():
    """vq(mdl, W) with W = the model's own columns returns mdl.select for distinct columns -- on the model's context, the data
    already resident; and vq(W, mdl) assigns every selected sample to itself."""
    rs = np.random.RandomState(5)
    data = rs.random_sample((12, 3000)).astype(np.float32)
    mdl = pymf_amd.SIVM(data, num_bases=6)
    mdl.factorize(niter=1)
    sel = np.asarray(mdl.select)
    assert len(set(sel.tolist())) == 6
    ctx = mdl._ctx
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pymf_amd.nmf.PrecisionWarning)              # (W is a float64 array)
        got = pymf_amd.vq(mdl, mdl.W)
        assert mdl._ctx is ctx and np.array_equal(got, sel)
        assert np.array_equal(pymf_amd.vq(mdl, data[:, sel], metric="l1"), sel)
        back = pymf_amd.vq(data[:, sel], mdl)
    assert np.array_equal(back[sel], np.arange(6))
    W0 = np.array(mdl.W)
    mdl.factorize(niter=1, compute_w=False)                                         # the context's own state was not touched
    assert np.array_equal(np.asarray(mdl.W), W0)


def test_c_abi_refusals():
    import scipy.sparse as sp
    rs = np.random.RandomState(2)
    V = rs.random_sample((6, 70)).astype(np.float32)
    Q = rs.random_sample((6, 129)).astype(np.float32)

    def refused(ctx, match, nq=3, metric=0):
        for call in (lambda: ctx.vq_columns(Q[:, :nq], metric), lambda: ctx.vq_assign(Q[:, :nq], metric)):
            with pytest.raises(_lib.PmfError, match=match) as ei:
                call()
            assert ei.value.code == _lib.PMF_EINVAL
    ctx = _lib.Context(_lib.ALGO_SIVM, 6, 70, 2)
    refused(ctx, "no dense data is resident")                                       # nothing set yet
    ctx.set_v_dense(V)
    refused(ctx, "1 <= nq <= 128", nq=129)
    refused(ctx, "metric 0 .l2. or 1 .l1.", metric=2)
    refused(ctx, "metric 0 .l2. or 1 .l1.", metric=-1)
    lib = _lib.load()
    q3 = np.ascontiguousarray(Q[:, :3])
    idx = np.zeros(70, dtype=np.int32)
    assert lib.pmf_vq_columns(ctx._h, q3.ctypes.data, 3, 0, 0, idx.ctypes.data, None) == _lib.PMF_EINVAL        # nq < 1
    assert lib.pmf_vq_assign(ctx._h, q3.ctypes.data, 3, 0, 0, idx.ctypes.data, None) == _lib.PMF_EINVAL
    assert lib.pmf_vq_columns(ctx._h, q3.ctypes.data, 2, 3, 0, idx.ctypes.data, None) == _lib.PMF_EINVAL        # ldq < nq
    assert lib.pmf_vq_assign(ctx._h, q3.ctypes.data, 3, 3, 0, None, None) == _lib.PMF_EINVAL                   # nothing asked for
    ci, _ = ctx.vq_columns(q3)                                                      # ... and the context still works
    assert np.array_equal(ci, np.argmin(vc.ref_pdist(q3, V, "l2"), axis=1))
    S = sp.random(6, 70, density=0.3, format="csc", random_state=3, dtype=np.float32)
    ctx.set_v_csc(S.indptr, S.indices, S.data)
    refused(ctx, "CSC data")
    ctx.close()
    ctx = _lib.Context(_lib.ALGO_SNMF, 6, 70, 2)
    R = S.tocsr()
    ctx.set_v_csr(R.indptr, R.indices, R.data)
    refused(ctx, "CSR data")
    ctx.close()
    ctx = _lib.Context(_lib.ALGO_NMF, 128, 70, 2)                                   # streamed: W and H set, tiles passing, no V
    ctx.set_w(rs.random_sample((128, 2)).astype(np.float32))
    ctx.set_h(rs.random_sample((2, 70)).astype(np.float32))
    Qs = rs.random_sample((128, 3)).astype(np.float32)
    ctx.stream_begin(max_tile_rows=64)
    ctx.stream_tile(0, rs.random_sample((64, 70)).astype(np.float32))
    for call in (lambda: ctx.vq_columns(Qs), lambda: ctx.vq_assign(Qs)):
        with pytest.raises(_lib.PmfError, match="streamed") as ei:
            call()
        assert ei.value.code == _lib.PMF_EINVAL
    ctx.stream_tile(64, rs.random_sample((64, 70)).astype(np.float32))
    ctx.stream_end()
    with pytest.raises(_lib.PmfError, match="streamed"):
        ctx.vq_columns(Qs)                                                          # (the pass is over: V was never resident)
    ctx.close()


def test_profile_sites():
    c = vc.exact(64, 257, 64)
    ctx = _lib.Context(_lib.ALGO_SIVM, c.m, c.n, 2)
    ctx.set_v_dense(c.V)
    for value, name, calls in ((1, "k_vq_pass<l1>", 2), (2, "k_vq_argmin_rows", 1)):
        ctx.set_option("profile_vq", value)
        ctx.profile_enable(True)
        ctx.vq_columns(c.Q, 1)
        ctx.vq_assign(c.Q, 1)
        st = ctx.kernel_stats()
        ctx.profile_enable(False)
        assert st["name"] == name and st["launches"] == calls and st["mean_ms"] > 0.0, st
    ctx.set_option("profile_vq", 0)
    ctx.profile_enable(True)
    ctx.update_w()
    assert ctx.kernel_stats()["name"] == "k_sivm_pass<l2>"
    ctx.close()
