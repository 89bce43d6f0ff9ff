"""pymf_amd.Kmeans / pymf_amd.Cmeans on scipy.sparse data (accept_sparse = True) on the MI355X against the float64 oracle on
toarray() (tests/cluster_oracle.py on the cases of tests/cluster_sparse_cases.py) and against the dense device run on toarray().
`assigned` and Kmeans' H exactly, W and H within the 2e-5 relative Frobenius of DESIGN.md section 4.  ferr within FACTOR x the
committed identity deviation (floored at 1e-13) relative to ||data||, against cluster_oracle.frobenius in float64 on toarray() and
the factors that the device returned.  The oracle's own trajectory keeps W in float64 where the device rounds it to float32 in
every W step; that enters ferr in first order (measured on the MI355X at 29 x 300: 3.0e-10 of ||data|| for Kmeans), so the
trajectory's ferr is compared at 2e-5 like W and H (tests/cluster_sparse_cases.py).  Every repetition bit-equal."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cluster_oracle as co
import cluster_sparse_cases as cs
import pymf_amd
from conftest import LEDGER_PATH, Measured
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 2e-5
_parity = {}


def within(value, tol, what):
    print("%-52s %.3e  (tol %.3e)" % (what, value, tol))
    _parity[what] = float(value)
    m = Measured(value)
    m.what = what
    return m <= tol


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    try:
        out = os.path.dirname(LEDGER_PATH)                    # beside the session's ledger; committed as profiles/parity_cluster_sparse.json
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_cluster_sparse.json"), "w") as f:
            json.dump({"achieved": _parity}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def kmeans_model(data, k, W0, sparse=True):
    mdl = pymf_amd.Kmeans(data, num_bases=k)
    mdl.accept_sparse = sparse
    mdl.W = np.array(W0)
    return mdl


def cmeans_model(data, k, W0, H0, sparse=True):
    mdl = pymf_amd.Cmeans(data, num_bases=k)
    mdl.accept_sparse = sparse
    mdl.W, mdl.H = np.array(W0), np.array(H0)
    return mdl


_runs = {}


def kmeans_run(name):
    if ("k", name) not in _runs:
        c = cs.case(name)
        mdl = kmeans_model(c["sparse"], c["num_bases"], c["W0"])
        mdl.factorize(niter=cs.NITER)
        _runs[("k", name)] = mdl
    return cs.case(name), _runs[("k", name)]


def cmeans_run(name):
    if ("c", name) not in _runs:
        c = cs.case(name)
        mdl = cmeans_model(c["sparse"], c["num_bases"], c["W0"], c["H0"])
        mdl.factorize(niter=cs.NITER)
        _runs[("c", name)] = mdl
    return cs.case(name), _runs[("c", name)]


# ---- 1: every case against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.SPARSE_CASES))
def test_kmeans_case_matches_the_oracle(name):
    c, mdl = kmeans_run(name)
    r = c["kmeans"]
    tag = "kmeans_sparse %s" % name
    assert mdl._ctx.path_name == "cluster_csr"
    assert mdl.assigned.dtype == np.intp and np.array_equal(mdl.assigned, r["assigned"]), "%d samples assigned differently" % int(
        np.sum(np.asarray(mdl.assigned) != r["assigned"]))
    assert type(mdl.H) is np.ndarray and mdl.H.dtype == np.float64 and np.array_equal(mdl.H, r["H"])
    assert type(mdl.W) is np.ndarray and within(rel(mdl.W, r["W"]), TOL, tag + " W")
    assert len(mdl.ferr) == len(r["ferr"]) and mdl.ferr[-1] != -123456
    direct = co.frobenius(c["d64"], mdl.W, mdl.H)
    f = mdl.frobenius_norm()                           # (the last entry of a history that converged() cut belongs to the iteration before)
    assert within(abs(f - direct) / c["norm"], cs.device_tol_ferr(), tag + " ferr vs direct on its factors")
    assert len(mdl.ferr) < cs.NITER or f == mdl.ferr[-1]
    print("%-52s %.3e" % (tag + " ferr vs oracle run / ||data||", np.max(np.abs(mdl.ferr - r["ferr"])) / c["norm"]))
    assert within(np.max(np.abs(mdl.ferr - r["ferr"]) / r["ferr"]), TOL, tag + " ferr vs oracle run")


@pytest.mark.parametrize("name", list(cs.SPARSE_CASES))
def test_cmeans_case_matches_the_oracle(name):
    c, mdl = cmeans_run(name)
    r = c["cmeans"]
    tag = "cmeans_sparse %s" % name
    assert mdl._ctx.path_name == "cluster_csr"
    assert type(mdl.H) is np.ndarray and mdl.H.dtype == np.float64 and mdl.H.shape == r["H"].shape
    assert within(rel(mdl.W, r["W"]), TOL, tag + " W")
    assert within(rel(mdl.H, r["H"]), TOL, tag + " H")
    assert len(mdl.ferr) == len(r["ferr"]) and mdl.ferr[-1] != -123456
    direct = co.frobenius(c["d64"], mdl.W, mdl.H)
    f = mdl.frobenius_norm()                           # (the last entry of a history that converged() cut belongs to the iteration before)
    assert within(abs(f - direct) / c["norm"], cs.device_tol_ferr(), tag + " ferr vs direct on its factors")
    assert len(mdl.ferr) < cs.NITER or f == mdl.ferr[-1]
    assert within(np.max(np.abs(mdl.ferr - r["ferr"]) / r["ferr"]), TOL, tag + " ferr vs oracle run")


@pytest.mark.parametrize("name", list(cs.SPARSE_CASES))
def test_the_dense_device_run_assigns_the_same(name):
    c, mdl = kmeans_run(name)
    dense = kmeans_model(c["data"], c["num_bases"], c["W0"], sparse=False)
    dense.factorize(niter=cs.NITER)
    assert dense._ctx.path_name == "cluster_panels"
    assert np.array_equal(dense.assigned, mdl.assigned) and np.array_equal(dense.H, mdl.H)
    assert rel(dense.W, mdl.W) < TOL and len(dense.ferr) == len(mdl.ferr)
    assert np.max(np.abs(dense.ferr - mdl.ferr) / mdl.ferr) < TOL


# ---- 2: more than 64 x 1024 samples: one H step, sample by sample ---------------------------------------------------------------
def test_wide_kmeans_sample_by_sample():
    c = cs.case(cs.WIDE_CASE)
    r = c["kmeans"]
    mdl = kmeans_model(c["sparse"], c["num_bases"], c["W0"])
    mdl.H = np.zeros((c["num_bases"], c["sparse"].shape[1]))
    mdl.update_h()
    a = np.asarray(mdl.assigned)
    n = a.shape[0]
    assert a.shape == r["assigned"].shape and a.min() >= 0 and a.max() < c["num_bases"]
    d = r["dist"]
    vn = np.sqrt((c["d64"] ** 2).sum(axis=0))
    excess = d[a, np.arange(n)] - d.min(axis=0)               # the oracle's distance of the device's centre above the minimum
    differ = int(np.sum(a != r["assigned"]))
    print("wide: %d of %d samples on another centre than the oracle's, largest excess / |v| %.3e" % (
        differ, n, float(np.max(np.where(vn > 0, excess / np.where(vn > 0, vn, 1.0), 0.0)))))
    ok = (a == r["assigned"]) | (excess <= 1e-4 * vn)
    assert np.all(ok), "%d samples beyond 1e-4 |v| of the nearest centre" % int(np.sum(~ok))
    assert np.array_equal(mdl.H, np.eye(c["num_bases"])[:, a]) and np.array_equal(np.argmax(mdl.H, axis=0), a)
    direct = co.frobenius(c["d64"], c["W32"], mdl.H)
    assert within(abs(mdl.frobenius_norm() - direct) / c["norm"], cs.device_tol_ferr(), "kmeans_sparse wide ferr vs direct on its factors")


def test_wide_cmeans_by_tolerance():
    c = cs.case(cs.WIDE_CASE)
    k, n = c["num_bases"], c["sparse"].shape[1]
    mdl = cmeans_model(c["sparse"], k, c["W0"], np.zeros((k, n)))
    mdl.update_h()
    assert within(rel(mdl.H, c["cmeans"]["H"]), TOL, "cmeans_sparse wide H")
    direct = co.frobenius(c["d64"], c["W32"], mdl.H)
    assert within(abs(mdl.frobenius_norm() - direct) / c["norm"], cs.device_tol_ferr(), "cmeans_sparse wide ferr vs direct on its factors")
    mdl.update_w()
    assert within(rel(mdl.W, co.cmeans_update_w(c["d64"], c["W32"], mdl.H)), TOL, "cmeans_sparse wide W")


# ---- 3: single hooks, partial loops ---------------------------------------------------------------------------------------------
def test_kmeans_single_hooks():
    c = cs.case("151x700_k8")
    d, k, n = c["d64"], c["num_bases"], c["sparse"].shape[1]
    W0 = c["W0"].astype(np.float32).astype(np.float64)
    mdl = kmeans_model(c["sparse"], k, W0)
    mdl.H = np.zeros((k, n))
    mdl.update_h()
    assigned, H, gap = co.kmeans_update_h(d, W0)
    assert np.array_equal(mdl.assigned, assigned) and np.array_equal(mdl.H, H)
    assert within(abs(mdl.frobenius_norm() - co.frobenius(d, W0, H)) / c["norm"], cs.device_tol_ferr(), "kmeans_sparse hook ferr")
    mdl.update_w()
    W1 = co.kmeans_update_w(d, W0, assigned)
    assert within(rel(mdl.W, W1), TOL, "kmeans_sparse hook update_w")
    assert within(abs(mdl.frobenius_norm() - co.frobenius(d, mdl.W, H)) / c["norm"], cs.device_tol_ferr(), "kmeans_sparse hook ferr after update_w")
    mdl.assigned = np.roll(assigned, 1)                # a caller's assignment is what update_w uses (kmeans.py:84)
    mdl.update_w()
    assert within(rel(mdl.W, co.kmeans_update_w(d, W1, np.roll(assigned, 1))), TOL, "kmeans_sparse hook update_w, caller's assigned")


def test_kmeans_update_w_without_an_assignment():
    c = cs.case("29x300_k5")
    mdl = kmeans_model(c["sparse"], c["num_bases"], c["W0"])
    mdl.H = np.zeros((c["num_bases"], 300))
    with pytest.raises(AttributeError):
        mdl.update_w()


def test_cmeans_single_hooks():
    c = cs.case("300x5000_k64")
    d, k = c["d64"], c["num_bases"]
    W0 = c["W0"].astype(np.float32).astype(np.float64)
    mdl = cmeans_model(c["sparse"], k, W0, c["H0"])
    assert within(abs(mdl.frobenius_norm() - co.frobenius(d, W0, c["H0"])) / c["norm"], cs.device_tol_ferr(), "cmeans_sparse hook ferr, caller's H")
    mdl.update_w()                                     # the sums of the caller's H: no pass preceded
    W1 = co.cmeans_update_w(d, W0, c["H0"])
    assert within(rel(mdl.W, W1), TOL, "cmeans_sparse hook update_w")
    mdl.W = np.array(W0)
    mdl.update_h()
    H1 = co.cmeans_update_h(d, W0)
    assert within(rel(mdl.H, H1), TOL, "cmeans_sparse hook update_h")
    assert np.allclose(mdl.H.sum(axis=0), 1.0, rtol=0, atol=1e-12)
    assert within(abs(mdl.frobenius_norm() - co.frobenius(d, W0, mdl.H)) / c["norm"], cs.device_tol_ferr(), "cmeans_sparse hook ferr")


@pytest.mark.parametrize("cw,ch", [(False, True), (True, False)])
def test_partial_loops(cw, ch):
    c = cs.case("1100x700_k6")
    d, k = c["d64"], c["num_bases"]
    W0 = c["W0"].astype(np.float32).astype(np.float64)        # (a W that no step rewrites is the device's only after this rounding)
    W, H, assigned, ferr, gap = co.kmeans(d, k, W=W0, niter=4, compute_w=cw, compute_h=ch)
    mdl = kmeans_model(c["sparse"], k, W0)
    mdl.factorize(niter=4, compute_w=cw, compute_h=ch)
    tag = "sparse cw=%s ch=%s" % (cw, ch)
    assert np.array_equal(mdl.assigned, assigned) and np.array_equal(mdl.H, H) and len(mdl.ferr) == len(ferr)
    assert within(rel(mdl.W, W), TOL, "kmeans_" + tag + " W")
    assert within(abs(mdl.frobenius_norm() - co.frobenius(d, mdl.W, mdl.H)) / c["norm"], cs.device_tol_ferr(), "kmeans_" + tag + " ferr")
    Wc, Hc, fc = co.cmeans(d, W0, c["H0"], niter=4, compute_w=cw, compute_h=ch)
    mdl = cmeans_model(c["sparse"], k, W0, c["H0"])
    mdl.factorize(niter=4, compute_w=cw, compute_h=ch)
    assert len(mdl.ferr) == len(fc)
    assert within(rel(mdl.W, Wc), TOL, "cmeans_" + tag + " W") and within(rel(mdl.H, Hc), TOL, "cmeans_" + tag + " H")
    assert within(abs(mdl.frobenius_norm() - co.frobenius(d, mdl.W, mdl.H)) / c["norm"], cs.device_tol_ferr(), "cmeans_" + tag + " ferr")


# ---- 4: centres with one member or none keep their column (kmeans.py:86) -------------------------------------------------------------
def test_small_clusters_keep_their_centre():
    rs = np.random.RandomState(11)
    V = (0.1 * rs.randn(16, 40)).astype(np.float32)
    V[:, :20] += 1.0                                   # two real clusters, around 1 and around 0 ...
    V[:, 7] = 10.0                                     # ... and one outlier
    V *= rs.rand(16, 40) < 0.7
    V[:, 7] = 10.0
    W0 = np.zeros((16, 4), dtype=np.float32)
    W0[:, 0] = 0.7
    W0[:, 2] = 9.75                                    # gets sample 7 alone
    W0[:, 3] = -50.0                                   # gets nobody
    W0 += (0.01 * rs.randn(16, 4)).astype(np.float32)
    W, H, assigned, ferr, gap = co.kmeans(V, 4, W=W0, niter=3)
    assert np.sum(assigned == 2) == 1 and np.sum(assigned == 3) == 0 and gap >= 1e-4
    mdl = kmeans_model(sp.csr_matrix(V), 4, W0.astype(np.float64))
    mdl.factorize(niter=3)
    assert np.array_equal(mdl.assigned, assigned) and np.array_equal(mdl.H, H) and len(mdl.ferr) == len(ferr)
    assert within(rel(mdl.W, W), TOL, "kmeans_sparse small clusters W")
    assert np.array_equal(mdl.W[:, 2:], W0[:, 2:].astype(np.float64))


# ---- 5: determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["151x700_k8", "300x5000_k64", "2100x4100_k128"])
def test_two_runs_give_the_same_bits(name):
    c, first = kmeans_run(name)
    mdl = kmeans_model(c["sparse"].copy(), c["num_bases"], c["W0"])
    mdl.factorize(niter=cs.NITER)
    assert np.array_equal(mdl.assigned, first.assigned) and np.array_equal(mdl.W, first.W) and np.array_equal(mdl.H, first.H)
    assert np.array_equal(mdl.ferr, first.ferr)
    c, first = cmeans_run(name)
    mdl = cmeans_model(c["sparse"].copy(), c["num_bases"], c["W0"], c["H0"])
    mdl.factorize(niter=cs.NITER)
    assert np.array_equal(mdl.W, first.W) and np.array_equal(mdl.H, first.H) and np.array_equal(mdl.ferr, first.ferr)


def test_float64_data_warns_once_and_any_format_is_taken():
    c, first = kmeans_run("29x300_k5")
    mdl = kmeans_model(c["sparse"].astype(np.float64).tocsc(), c["num_bases"], c["W0"])
    with pytest.warns(pymf_amd.nmf.PrecisionWarning):
        mdl.factorize(niter=cs.NITER)
    assert np.array_equal(mdl.assigned, first.assigned) and np.array_equal(mdl.W, first.W) and np.array_equal(mdl.ferr, first.ferr)
    coo = cmeans_model(c["sparse"].tocoo(), c["num_bases"], c["W0"], c["H0"])
    coo.factorize(niter=cs.NITER)
    assert np.array_equal(coo.W, cmeans_run("29x300_k5")[1].W)


def test_init_w_and_init_h_run_on_sparse_data():
    import random
    c = cs.case("151x700_k8")
    random.seed(5)
    mdl = pymf_amd.Kmeans(c["sparse"], num_bases=c["num_bases"])
    mdl.accept_sparse = True
    mdl.factorize(niter=2)
    random.seed(5)
    dense = pymf_amd.Kmeans(c["data"], num_bases=c["num_bases"])
    dense.factorize(niter=2)
    assert type(mdl.W) is np.ndarray and mdl.W.shape == dense.W.shape and mdl.assigned.shape == (700,)
    assert within(abs(mdl.ferr[-1] - co.frobenius(c["d64"], mdl.W, mdl.H)) / c["norm"], cs.device_tol_ferr(), "kmeans_sparse own init ferr")
    np.random.seed(5)
    cm = pymf_amd.Cmeans(c["sparse"], num_bases=c["num_bases"])
    cm.accept_sparse = True
    cm.factorize(niter=2)
    assert within(abs(cm.ferr[-1] - co.frobenius(c["d64"], cm.W, cm.H)) / c["norm"], cs.device_tol_ferr(), "cmeans_sparse own init ferr")


# ---- 6: the context -----------------------------------------------------------------------------------------------------------------
def csr_context(name, algo=_lib.ALGO_KMEANS):
    c = cs.case(name)
    A = c["sparse"]
    ctx = _lib.Context(algo, A.shape[0], A.shape[1], c["num_bases"])
    ctx.set_v_csr(A.indptr, A.indices, A.data)
    return c, A, ctx


@pytest.mark.parametrize("algo", [_lib.ALGO_KMEANS, _lib.ALGO_CMEANS])
def test_sparse_dense_sparse_on_one_context(algo):
    c, A, ctx = csr_context("151x700_k8", algo)
    try:
        def run():
            ctx.set_w(c["W0"])
            if algo == _lib.ALGO_CMEANS:
                ctx.set_h(c["H0"])
                ctx.update_w()
            ctx.update_h()
            ctx.update_w()
            ctx.update_h()
            return ctx.get_w(), ctx.get_h64(), ctx.frobenius()

        assert ctx.path_name == "cluster_csr"
        W1, H1, f1 = run()
        a1 = ctx.get_assigned() if algo == _lib.ALGO_KMEANS else None
        ctx.set_v_dense(c["data"])
        assert ctx.path_name == "cluster_panels"
        assert rel(ctx.get_h64(), H1) <= 1e-6                  # H survives the change of the data, rounded to float32
        W2, H2, f2 = run()
        assert rel(W2, W1) < TOL and rel(H2, H1) < TOL and abs(f2 - f1) <= TOL * f1
        if a1 is not None:
            assert np.array_equal(ctx.get_assigned(), a1) and np.array_equal(H2, H1)
        ctx.set_v_csr(A.indptr, A.indices, A.data)
        assert ctx.path_name == "cluster_csr"
        assert rel(ctx.get_h64(), H2) <= 1e-6                  # ... and back, widened
        W3, H3, f3 = run()
        assert np.array_equal(W3, W1) and np.array_equal(H3, H1) and f3 == f1
        if a1 is not None:
            assert np.array_equal(ctx.get_assigned(), a1)
    finally:
        ctx.close()


def test_malformed_arrays_are_refused_with_the_resident_data_intact():
    c, A, ctx = csr_context("29x300_k5")
    try:
        ctx.set_w(c["W0"])
        ctx.update_h()
        want = ctx.get_assigned()
        swapped = A.indices.copy()
        r = int(np.argmax(np.diff(A.indptr) >= 2))
        lo = A.indptr[r]
        swapped[lo], swapped[lo + 1] = swapped[lo + 1], swapped[lo]
        dup = A.indices.copy()
        dup[lo + 1] = dup[lo]
        bad_ptr = A.indptr.copy()
        bad_ptr[3] = bad_ptr[4] + 1
        out = A.indices.copy()
        out[0] = 300
        for ip, ind, why in ((A.indptr, swapped, "ascend"), (A.indptr, dup, "ascend"), (bad_ptr, A.indices, "indptr"), (A.indptr, out, "out of range")):
            with pytest.raises(_lib.PmfError, match="pmf_set_v_csr_f32: .*" + why) as ei:
                ctx.set_v_csr(ip, ind, A.data)
            assert ei.value.code == _lib.PMF_EINVAL
        assert ctx.path_name == "cluster_csr"
        ctx.update_h()
        assert np.array_equal(ctx.get_assigned(), want)
    finally:
        ctx.close()


def test_entry_points_without_a_csr_form():
    c, A, ctx = csr_context("29x300_k5")
    try:
        calls = [lambda: ctx.fill_w_uniform(1), lambda: ctx.fill_h_uniform(2), lambda: ctx.snapshot_w(), lambda: ctx.snapshot_h(),
                 lambda: ctx.stream_begin(max_tile_rows=64, compute_w=True), lambda: ctx.nndsvd_init()]
        for call in calls:
            with pytest.raises(_lib.PmfError, match="not while CSR data is resident on a Kmeans / Cmeans context") as ei:
                call()
            assert ei.value.code == _lib.PMF_EINVAL
        ctx.set_w(c["W0"])                                     # ... and the context still works
        ctx.update_h()
        assert np.array_equal(ctx.get_assigned(), co.kmeans_update_h(c["d64"], c["W0"])[0])
    finally:
        ctx.close()


@pytest.mark.parametrize("name,algo,tag", [("300x5000_k64", _lib.ALGO_KMEANS, "<1,kmeans>"), ("2100x4100_k128", _lib.ALGO_CMEANS, "<2,cmeans>")])
def test_the_profile_record_names_the_launched_instantiation(name, algo, tag):
    c, A, ctx = csr_context(name, algo)
    try:
        k, n, ld = c["num_bases"], A.shape[1], 64 if c["num_bases"] <= 64 else 128
        ctx.set_w(c["W0"])
        ctx.profile_enable(True)
        ctx.update_h()
        st = ctx.kernel_stats()
        print(st)
        assert st["name"] == "k_cluster_csr_assign" + tag and st["launches"] == 1 and st["mean_ms"] > 0
        assert st["flops_per_launch"] == 2.0 * A.nnz * k
        assert st["bytes_per_launch"] == 8.0 * A.nnz + 16.0 * n + 8.0 * ld * n + (4.0 * n if algo == _lib.ALGO_KMEANS else 0.0)
        ctx.profile_enable(True)
        ctx.update_w()
        st = ctx.kernel_stats()
        print(st)
        assert st["name"] == "k_cluster_csr_num" + tag and st["launches"] == 1 and st["mean_ms"] > 0
        assert st["flops_per_launch"] == 2.0 * A.nnz * k
    finally:
        ctx.close()


@pytest.mark.parametrize("cls", ["Kmeans", "Cmeans"])
def test_129_bases_are_refused(cls):
    mdl = getattr(pymf_amd, cls)(cs.case("29x300_k5")["sparse"], num_bases=129)
    mdl.accept_sparse = True
    with pytest.raises(ValueError):
        mdl.factorize(niter=1)
    with pytest.raises(_lib.PmfError):
        _lib.Context(_lib.ALGO_KMEANS if cls == "Kmeans" else _lib.ALGO_CMEANS, 29, 300, 129)
