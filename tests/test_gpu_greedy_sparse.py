"""pymf_amd.GREEDY on scipy.sparse data (accept_sparse = True) on the MI355X against the float64 oracle on toarray()
(tests/greedy_oracle.py on the cases of tests/greedy_sparse_cases.py), against the dense device run on toarray() and against the
goldens of the reference's own sparse branch.  `select` exactly, W bit-equal to the data's columns, H within
greedy_cases.device_tol_h(), ferr within FACTOR x the committed identity deviation (floored at 1e-13) relative to ||data||; every
repetition bit-equal."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import greedy_cases as gc
import greedy_oracle as go
import greedy_sparse_cases as gs
import pymf_amd
from conftest import LEDGER_PATH, Measured
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_parity = {}


def within(value, tol, what):
    print("%-40s %.3e  (tol %.3e)" % (what, value, tol))
    _parity[what] = float(value)
    m = Measured(value)
    m.what = what
    return m <= tol


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    try:
        out = os.path.dirname(LEDGER_PATH)                    # beside the session's ledger; committed as profiles/parity_greedy_sparse.json
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_greedy_sparse.json"), "w") as f:
            json.dump({"achieved": _parity}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def model(data, k, sparse=True):
    mdl = pymf_amd.GREEDY(data, num_bases=k)
    mdl.accept_sparse = sparse
    return mdl


_runs = {}


def sparse_run(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _runs:
        c = gs.case(name)
        np.random.seed(3)
        mdl = model(c["sparse"], c["num_bases"])
        mdl.factorize(**kw)
        _runs[key] = mdl
    return gs.case(name), _runs[key]


@pytest.mark.parametrize("name", gs.h_cases())
def test_case_matches_the_oracle(name):
    c, mdl = sparse_run(name)
    assert mdl._ctx.path_name == "greedy_csr"
    assert mdl.select == c["select"] and all(type(s) is int for s in mdl.select)
    assert type(mdl.W) is np.ndarray and mdl.W.dtype == np.float32 and np.array_equal(mdl.W, c["data"][:, c["select"]])
    assert type(mdl.H) is np.ndarray and mdl.H.dtype == np.float64 and mdl.H.shape == c["H"].shape
    assert within(gc.rel_max(mdl.H, c["H"]), gc.device_tol_h(), "greedy_sparse %s H" % name)
    assert mdl.ferr.shape == (1,) and mdl.ferr[0] != -123456
    assert within(abs(mdl.ferr[0] - c["ferr"]) / c["norm"], gs.device_tol_ferr(), "greedy_sparse %s ferr" % name)
    assert mdl.frobenius_norm() == mdl.ferr[0]


def test_planted_tie_takes_the_lower_index():
    c, mdl = sparse_run(gs.TIE_CASE)
    m, n, _, density, seed = gs.TIE_BASE
    src, dup = gs.tie_columns(gs.raw_matrix(m, n, density, seed).toarray())
    assert mdl.select[0] == src and dup not in mdl.select and mdl.select == c["select"]


def test_rank_deficient_data():
    c, mdl = sparse_run(gs.RANK_CASE, compute_h=False, compute_err=False)
    print(mdl.select, c["select"])
    assert mdl.select[:gs.RANK - 1] == c["select"][:gs.RANK - 1]
    T = c["scores"][gs.RANK - 1]
    assert T[mdl.select[gs.RANK - 1]] >= T.max() * (1.0 - gc.TIE_RTOL)
    assert len(mdl.select) == 5 and len(set(mdl.select)) == 5 and all(0 <= s < 300 for s in mdl.select)
    assert np.array_equal(mdl.W, c["data"][:, mdl.select])


@pytest.mark.parametrize("name", ["29x300_k6", "300x29_k6"])
def test_the_reference_sparse_branch(name):
    g = np.load(os.path.join(GOLD, "greedy_sparse_%s.npz" % name))
    _, mdl = sparse_run(name)
    assert mdl.select == [int(s) for s in g["select"]]


@pytest.mark.parametrize("name", ["29x300_k6", "151x700_k8", "80x640_k64", "300x29_k6", "200x200_k10"])
def test_the_dense_device_run_selects_the_same(name):
    c, mdl = sparse_run(name)
    np.random.seed(3)
    dense = model(c["data"], c["num_bases"], sparse=False)
    dense.factorize()
    assert dense._ctx.path_name == "greedy_panels"
    assert dense.select == mdl.select and np.array_equal(dense.W, mdl.W)
    assert gc.rel_max(mdl.H, dense.H) <= 2 * gc.device_tol_h()
    assert abs(mdl.ferr[0] - dense.ferr[0]) <= (gc.device_tol_ferr() + gs.device_tol_ferr()) * c["norm"]


def csr_context(name, k=None):
    c = gs.case(name)
    A = c["sparse"]
    ctx = _lib.Context(_lib.ALGO_GREEDY, A.shape[0], A.shape[1], k or c["num_bases"])
    ctx.set_v_csr(A.indptr, A.indices, A.data)
    return c, A, ctx


@pytest.mark.parametrize("name", gs.TRANSPOSED)
def test_transposed_selection(name):
    """pmf_greedy_select(transposed = 1) on CSR data: the candidates are the rows, lines of the image of V; no transposed copy."""
    c, A, ctx = csr_context(name)
    try:
        k = c["num_bases"]
        assert ctx.greedy_select(k, transposed=True).tolist() == c["select_t"]
        assert ctx.greedy_select(k).tolist() == c["select"]
        assert ctx.greedy_select(k, transposed=True).tolist() == c["select_t"]
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["151x700_k8", "80x640_k64", "2100x64_k12"])
def test_two_runs_give_the_same_bits(name):
    c, first = sparse_run(name)
    np.random.seed(3)
    mdl = model(c["sparse"].copy(), c["num_bases"])
    mdl.factorize()
    assert mdl.select == first.select and np.array_equal(mdl.W, first.W) and np.array_equal(mdl.H, first.H)
    assert np.array_equal(mdl.ferr, first.ferr)
    mdl.factorize()                                            # ... and again on the same object and context
    assert mdl.select == first.select and np.array_equal(mdl.H, first.H) and np.array_equal(mdl.ferr, first.ferr)


def test_hooks_by_hand_and_niter3():
    c, first = sparse_run("151x700_k8")
    hand = model(c["sparse"], c["num_bases"])
    hand.update_w()
    hand.update_h()
    assert hand.select == first.select and np.array_equal(hand.W, first.W) and np.array_equal(hand.H, first.H)
    assert hand.frobenius_norm() == first.ferr[0]
    loop = model(c["sparse"], c["num_bases"])
    loop.factorize(niter=3)                                    # nmf.py:198-202: both updates repeat themselves, the loop stops at i = 2
    assert loop.ferr.shape == (2,) and loop.ferr[0] == loop.ferr[1] == first.ferr[0] and loop.select == first.select


def test_float64_data_warns_once_and_keeps_its_dtype():
    c = gs.case("29x300_k6")
    mdl = model(c["sparse"].astype(np.float64).tocsc(), c["num_bases"])
    with pytest.warns(pymf_amd.nmf.PrecisionWarning):
        mdl.factorize()
    assert mdl.select == c["select"] and mdl.W.dtype == np.float64
    assert np.array_equal(mdl.W, c["data"][:, c["select"]].astype(np.float64))
    assert within(gc.rel_max(mdl.H, c["H"]), gc.device_tol_h(), "greedy_sparse 29x300_k6 float64 csc H")


def test_sparse_dense_sparse_on_one_context():
    c, A, ctx = csr_context("151x700_k8")
    try:
        def run():
            ctx.update_w()
            ctx.update_h()
            return ctx.get_select().tolist(), ctx.get_w(), ctx.get_h64(), ctx.frobenius()

        assert ctx.path_name == "greedy_csr"
        s1, W1, H1, f1 = run()
        assert s1 == c["select"]
        ctx.set_v_dense(c["data"])
        assert ctx.path_name == "greedy_panels"
        assert gc.rel_max(ctx.get_h64(), H1) <= 1e-6           # H survives the change of the data, rounded to float32
        s2, W2, H2, f2 = run()
        assert s2 == s1 and np.array_equal(W2, W1) and gc.rel_max(H2, H1) <= 2 * gc.device_tol_h()
        ctx.set_v_csr(A.indptr, A.indices, A.data)
        assert ctx.path_name == "greedy_csr"
        s3, W3, H3, f3 = run()
        assert s3 == s1 and np.array_equal(W3, W1) and np.array_equal(H3, H1) and f3 == f1
    finally:
        ctx.close()


def test_malformed_arrays_are_refused_with_the_resident_data_intact():
    c, A, ctx = csr_context("29x300_k6")
    try:
        ctx.update_w()
        want = ctx.get_select().tolist()
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
        assert ctx.path_name == "greedy_csr" and ctx.greedy_select(c["num_bases"]).tolist() == want == c["select"]
    finally:
        ctx.close()
    big = _lib.Context(_lib.ALGO_GREEDY, 1025, 1100, 2)
    try:
        with pytest.raises(_lib.PmfError, match="1024") as ei:
            big.set_v_csr(np.zeros(1026, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
        assert ei.value.code == _lib.PMF_EINVAL
    finally:
        big.close()


def test_entry_points_without_a_csr_form():
    c, A, ctx = csr_context("29x300_k6")
    try:
        calls = [lambda: ctx.fill_w_uniform(1), lambda: ctx.fill_h_uniform(2), lambda: ctx.snapshot_w(), lambda: ctx.snapshot_h(),
                 lambda: ctx.stream_begin(max_tile_rows=64, compute_w=True), lambda: ctx.nndsvd_init()]
        for call in calls:
            with pytest.raises(_lib.PmfError, match="not while CSR data is resident on a GREEDY context") as ei:
                call()
            assert ei.value.code == _lib.PMF_EINVAL
        ctx.update_w()                                         # ... and the context still works
        assert ctx.get_select().tolist() == c["select"]
    finally:
        ctx.close()


def test_the_profile_record_of_the_pass():
    c, A, ctx = csr_context("80x640_k64")
    try:
        ctx.profile_enable(True)
        ctx.update_w()
        st = ctx.kernel_stats()
        print(st)
        cc = 64                                                # (the Gram matrix has at least 64 eigenvalues above the cut: test_greedy_sparse_cases.py)
        assert st["name"] == "k_greedy_csr_pass<2>" and st["launches"] == 64 and st["mean_ms"] > 0
        assert st["flops_per_launch"] == 2.0 * A.nnz * (cc + 63)
        assert st["bytes_per_launch"] == 12.0 * A.nnz + 8.0 * 640 + 4.0 * 128 * 80
        assert ctx.get_select().tolist() == c["select"]
    finally:
        ctx.close()
