"""pymf_amd.CUR / CMD on scipy.sparse data (accept_sparse = True) on the MI355X against the float64 oracle on toarray()
(tests/cur_oracle.py on the cases of tests/cur_sparse_cases.py) and against the dense device run on toarray().  The draws must
equal the oracle's exactly; the norms within test_gpu_cur.py's SQNORM_RTOL; C and R the data's rows and columns times
sqrt(count) to 1 ulp and bit-equal to the dense run's; the middle factor within tol_U = (kappa_C + kappa_R) x 1e-9 of the
oracle and 2 tol_U of the dense run; frobenius_norm within 4 x the deviation of the trace identity from the direct error
(floored at 1e-13; tests/golden/cur_sparse_tolerances.json)."""
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import cur_cases as cc
import cur_oracle as co
import cur_sparse_cases as scs
import pymf_amd
from conftest import LEDGER_PATH, Measured
from pymf_amd import _lib
from test_gpu_cur import SQNORM_RTOL

pytestmark = pytest.mark.gpu

CLASSES = {"cur": pymf_amd.CUR, "cmd": pymf_amd.CMD}
PAIRS = [(name, kind) for name in sorted(scs.SPARSE_CASES) for kind in scs.KINDS]

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
        out = os.path.dirname(LEDGER_PATH)                    # beside the session's ledger; committed as profiles/parity_cur_sparse.json
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_cur_sparse.json"), "w") as f:
            json.dump({"achieved": _parity}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def factorize(name, kind, data=None, sparse=True):
    c = scs.case(name, kind)
    if data is None:
        data = c["sparse"] if sparse else c["data"]
    mdl = CLASSES[kind](data, rrank=c["rrank"])
    mdl.accept_sparse = sparse
    np.random.seed(c["seed"])
    mdl.factorize()
    return mdl


_runs = {}


def device_run(name, kind, sparse=True):
    if (name, kind, sparse) not in _runs:
        _runs[(name, kind, sparse)] = factorize(name, kind, sparse=sparse)
    return scs.case(name, kind), _runs[(name, kind, sparse)]


def one_ulp(got, want):
    return bool(np.all(np.abs(got - want) <= np.spacing(np.abs(want))))


def sqnorm_dev(got, want):
    """max relative deviation over the lines with entries; the empty lines must be exactly 0"""
    assert np.array_equal(got == 0.0, want == 0.0)
    nz = want != 0.0
    return float(np.max(np.abs(got[nz] - want[nz]) / want[nz]))


@pytest.mark.parametrize("name,kind", PAIRS)
def test_parity(name, kind):
    c, mdl = device_run(name, kind)
    _, dense = device_run(name, kind, sparse=False)
    tag = "sparse %s %s " % (kind, name)
    d64 = c["data"].astype(np.float64)
    assert mdl._context().path_name == "cur_csr" and dense._context().path_name == "cur_cross_f64"
    # sampling
    for q in ("rid", "cid", "rcnt", "ccnt"):
        assert np.array_equal(np.asarray(getattr(mdl, "_" + q), dtype=np.float64), c[q].astype(np.float64)), q
        assert np.array_equal(np.asarray(getattr(mdl, "_" + q)), np.asarray(getattr(dense, "_" + q))), q
    row_sq, col_sq = mdl._context().cur_sqnorms()
    drow, dcol = dense._context().cur_sqnorms()
    sq = d64 ** 2
    dn = max(sqnorm_dev(row_sq, sq.sum(axis=1)), sqnorm_dev(col_sq, sq.sum(axis=0)))
    dnd = max(sqnorm_dev(row_sq, drow), sqnorm_dev(col_sq, dcol))
    # factors: dense float64 arrays
    assert mdl.U is mdl._C and mdl.S is mdl._U and mdl.V is mdl._R
    for a in (mdl.U, mdl.S, mdl.V):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64
    assert mdl.U.shape == c["C"].shape and mdl.S.shape == c["U"].shape and mdl.V.shape == c["R"].shape
    assert one_ulp(mdl.U, d64[:, c["cid"]] * np.sqrt(c["ccnt"])) and one_ulp(mdl.V, np.sqrt(c["rcnt"])[:, None] * d64[c["rid"], :])
    assert np.array_equal(mdl.U, dense.U) and np.array_equal(mdl.V, dense.V)
    # middle factor
    du, dud = cc.rel_max(mdl.S, c["U"]), cc.rel_max(mdl.S, dense.S)
    # error
    f = mdl.frobenius_norm()
    dfn, dfd = abs(f - c["ferr"]) / c["norm"], abs(f - dense.frobenius_norm()) / c["norm"]
    print("%snorms %.3e dense %.3e (tol %.1e)  U %.3e dense %.3e (tol_U %.3e)  frobenius_norm %.3e (tol %.3e) dense %.3e (tol %.3e)" % (
        tag, dn, dnd, SQNORM_RTOL, du, dud, c["tol_U"], dfn, scs.device_tol_ferr(), dfd, scs.device_tol_ferr_dense()))
    assert measured(dn, tag + "sqnorms") <= SQNORM_RTOL
    assert measured(dnd, tag + "sqnorms dense") <= SQNORM_RTOL
    assert measured(du, tag + "U") <= c["tol_U"]
    assert measured(dud, tag + "U dense") <= 2 * c["tol_U"]
    assert measured(dfn, tag + "frobenius_norm") <= scs.device_tol_ferr()
    assert measured(dfd, tag + "frobenius_norm dense") <= scs.device_tol_ferr_dense()


def with_duplicates(A, fmt):
    """A as a coo_matrix whose first 40 entries are split in two halves, in the given format where that keeps them apart."""
    coo = A.tocoo()
    k = min(40, coo.nnz)
    half = (coo.data[:k] * np.float32(0.5)).astype(np.float32)     # (exact: a power of two; the halves add up to the value)
    row = np.concatenate([coo.row, coo.row[:k]])
    col = np.concatenate([coo.col, coo.col[:k]])
    val = np.concatenate([half, coo.data[k:], half])
    dup = sp.coo_matrix((val, (row, col)), shape=A.shape)
    return dup if fmt == "coo" else dup.asformat(fmt)


@pytest.mark.parametrize("name", ["29x300", "2100x130"])
def test_input_formats_same_bits(name):
    c, mdl = device_run(name, "cur")
    for fmt in ("csr", "csc", "coo"):
        data = with_duplicates(c["sparse"], fmt)
        if fmt == "coo":
            assert data.nnz > c["sparse"].nnz                      # the duplicates are still apart
        assert np.array_equal(data.toarray(), c["data"])
        other = factorize(name, "cur", data=data)
        assert np.array_equal(other._rid, mdl._rid) and np.array_equal(other._cid, mdl._cid)
        assert np.array_equal(other.U, mdl.U) and np.array_equal(other.S, mdl.S) and np.array_equal(other.V, mdl.V), fmt
        assert other.frobenius_norm() == mdl.frobenius_norm()


@pytest.mark.parametrize("name", ["130x2100", "2100x130", "3000x2500"])
def test_two_runs_same_bits(name):
    for kind in scs.KINDS:
        c, mdl = device_run(name, kind)
        again = factorize(name, kind)
        assert np.array_equal(again.U, mdl.U) and np.array_equal(again.S, mdl.S) and np.array_equal(again.V, mdl.V)
        assert again.frobenius_norm() == mdl.frobenius_norm()
        U, S, V, f = mdl.U, mdl.S, mdl.V, mdl.frobenius_norm()
        np.random.seed(c["seed"])
        mdl.factorize()                                        # the same object, the same context
        assert np.array_equal(mdl.U, U) and np.array_equal(mdl.S, S) and np.array_equal(mdl.V, V) and mdl.frobenius_norm() == f
        p1, p2 = mdl._context().cur_sqnorms(), again._context().cur_sqnorms()
        assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])


@pytest.mark.parametrize("name", ["130x2100", "2100x130"])
def test_compute_ucr_with_indices_set_by_hand(name):
    """computeUCR() alone: the full line, an empty line, a repeated index, negative indices, counts above 1; then nr = nc = 1."""
    c = scs.case(name, "cur")
    d64 = c["data"].astype(np.float64)
    rows, cols = d64.shape
    rid, rcnt = np.array([rows // 3, 7, rows // 2, 7, -1, 3]), np.array([1.0, 2.0, 1.0, 1.0, 3.0, 1.0])   # rows // 2 and -1 are empty
    cid, ccnt = np.array([cols // 3, cols // 2, -2, 17, 5]), np.array([1.0, 1.0, 3.0, 1.0, 2.0])          # cols // 2 is empty
    rid_pos, cid_pos = np.where(rid < 0, rid + rows, rid), np.where(cid < 0, cid + cols, cid)
    C, U, R = co.compute_ucr(d64, rid_pos, rcnt, cid_pos, ccnt)
    gram = co.gram_form(d64, rid_pos, rcnt, cid_pos, ccnt)
    assert min(gram["kept_c"].min(), gram["kept_r"].min()) >= 1e-3
    assert max(np.abs(gram["dropped_c"]).max(initial=0.0), np.abs(gram["dropped_r"]).max(initial=0.0)) <= 1e-10
    assert gram["dropped_r"].size == 3 and gram["dropped_c"].size == 1       # the repeated row, two empty rows; the empty column
    tol_u = (cc.cond(gram["kept_c"]) + cc.cond(gram["kept_r"])) * cc.JACOBI_RTOL
    mdl = pymf_amd.CUR(c["sparse"], rrank=6)
    mdl.accept_sparse = True
    mdl._rid, mdl._rcnt, mdl._cid, mdl._ccnt = rid, rcnt, cid, ccnt
    mdl.computeUCR()
    assert mdl.S.shape == (5, 6) and one_ulp(mdl.U, C) and one_ulp(mdl.V, R)
    assert not mdl.V[2].any() and not mdl.V[4].any() and not mdl.U[:, 1].any()
    assert not mdl.S[:, 2].any() and not mdl.S[:, 4].any() and not mdl.S[1].any()    # an empty line: a zero column / row of U
    du = cc.rel_max(mdl.S, U)
    dfn = abs(mdl.frobenius_norm() - co.ferr(d64, C, U, R)) / c["norm"]
    print("sparse %s by hand: U %.3e (tol %.3e) frobenius_norm %.3e (tol %.3e)" % (name, du, tol_u, dfn, scs.device_tol_ferr()))
    assert measured(du, "sparse %s by hand U" % name) <= tol_u
    assert measured(dfn, "sparse %s by hand frobenius_norm" % name) <= scs.device_tol_ferr()
    # a rebound factor cannot be evaluated without a dense image
    keep = mdl.S
    mdl.S = np.zeros_like(mdl.S)
    with pytest.raises(NotImplementedError, match="S was rebound"):
        mdl.frobenius_norm()
    mdl.S = keep
    # one row, one column (the full ones), on the same context
    mdl._rid, mdl._rcnt, mdl._cid, mdl._ccnt = np.array([rows // 3]), np.array([2.0]), np.array([cols // 3]), np.array([1.0])
    mdl.computeUCR()
    C1, U1, R1 = co.compute_ucr(d64, mdl._rid, mdl._rcnt, mdl._cid, mdl._ccnt)
    assert mdl.S.shape == (1, 1) and one_ulp(mdl.U, C1) and one_ulp(mdl.V, R1)
    assert measured(cc.rel_max(mdl.S, U1), "sparse %s 1x1 U" % name) <= 2 * cc.JACOBI_RTOL
    assert measured(abs(mdl.frobenius_norm() - co.ferr(d64, C1, U1, R1)) / c["norm"], "sparse %s 1x1 frobenius_norm" % name) <= scs.device_tol_ferr()


def test_stored_zeros_are_zeros():
    c, mdl = device_run("29x300", "cur")
    A = c["sparse"].tocoo()
    rows, cols = A.shape
    # explicit zeros: into the two empty rows and an empty column, kept as stored entries
    zr, zc = np.array([rows // 2, rows - 1, 3]), np.array([5, 9, cols // 2])
    B = sp.csr_matrix((np.concatenate([A.data, np.zeros(3, dtype=np.float32)]), (np.concatenate([A.row, zr]), np.concatenate([A.col, zc]))),
                      shape=A.shape)
    assert B.nnz == A.nnz + 3 and np.array_equal(B.toarray(), c["data"])
    other = factorize("29x300", "cur", data=B)
    assert np.array_equal(other._rid, mdl._rid) and np.array_equal(other._cid, mdl._cid)
    assert np.array_equal(other.U, mdl.U) and np.array_equal(other.S, mdl.S) and np.array_equal(other.V, mdl.V)
    assert other.frobenius_norm() == mdl.frobenius_norm()
    r1, c1 = other._context().cur_sqnorms()
    assert r1[rows // 2] == 0.0 and r1[rows - 1] == 0.0 and c1[cols // 2] == 0.0


def test_float64_data_warns_once():
    c = scs.case("37x29", "cur")
    mdl = pymf_amd.CUR(c["sparse"].astype(np.float64), rrank=5)
    mdl.accept_sparse = True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        np.random.seed(c["seed"])
        mdl.factorize()
        mdl.factorize()
    assert len([x for x in w if issubclass(x.category, pymf_amd.nmf.PrecisionWarning)]) == 1


def test_cabi_alone():
    c = scs.case("37x29", "cmd")
    A = c["sparse"]
    m, n = A.shape
    k = len(c["rid"])
    tol_f = scs.device_tol_ferr() * c["norm"]
    ctx = _lib.Context(_lib.ALGO_CUR, m, n, max(k, len(c["cid"])))

    def run_sparse():
        ctx.set_v_csr(A.indptr, A.indices, A.data)
        assert ctx.path_name == "cur_csr"
        ctx._cur_shape = (1, 1)
        with pytest.raises(_lib.PmfError):
            ctx.cur_get()                                      # nothing decomposed yet
        with pytest.raises(_lib.PmfError):
            ctx.cur_ferr()
        row_sq, col_sq = ctx.cur_sqnorms()
        sq = c["data"].astype(np.float64) ** 2
        assert sqnorm_dev(row_sq, sq.sum(axis=1)) <= SQNORM_RTOL and sqnorm_dev(col_sq, sq.sum(axis=0)) <= SQNORM_RTOL
        ctx.cur_compute(c["rid"], c["rcnt"], c["cid"], c["ccnt"])
        C, U, R = ctx.cur_get()
        assert cc.rel_max(U, c["U"]) <= c["tol_U"] and one_ulp(C, c["C"]) and one_ulp(R, c["R"])
        assert abs(ctx.cur_ferr() - c["ferr"]) <= tol_f
        return C, U, R, ctx.cur_ferr()

    first = run_sparse()
    # the entry points without a CSR form say so
    for call in (lambda: ctx.cur_leverage(2, 2), ctx.frobenius, lambda: ctx.factorize(1), ctx.update_w):
        with pytest.raises(_lib.PmfError) as ei:
            call()
        assert ei.value.code == _lib.PMF_EINVAL
    for call in (lambda: ctx.cur_leverage(2, 2), ctx.frobenius):
        with pytest.raises(_lib.PmfError, match="CSR data is resident"):
            call()
    # malformed arrays are refused on the host, and the resident data stay
    unsorted = A.indices.copy()
    r = int(np.argmax(np.diff(A.indptr) >= 2))
    lo = A.indptr[r]
    unsorted[lo], unsorted[lo + 1] = unsorted[lo + 1], unsorted[lo]
    repeated = A.indices.copy()
    repeated[lo + 1] = repeated[lo]
    outside = A.indices.copy()
    outside[lo] = n
    falling = A.indptr.copy()
    falling[r + 1], falling[r + 2] = falling[r + 2] + 1, falling[r + 1]
    for ip, ind, why in ((A.indptr, unsorted, "must ascend"), (A.indptr, repeated, "must ascend"), (A.indptr, outside, "out of range"),
                         (falling, A.indices, "must not decrease")):
        with pytest.raises(_lib.PmfError, match="pmf_set_v_csr_f32: .*" + why) as ei:
            ctx.set_v_csr(ip, ind, A.data)
        assert ei.value.code == _lib.PMF_EINVAL
    assert ctx.path_name == "cur_csr"
    C, U, R = ctx.cur_get()
    assert np.array_equal(U, first[1]) and ctx.cur_ferr() == first[3]
    ctx.cur_compute(c["rid"], c["rcnt"], c["cid"], c["ccnt"])
    assert np.array_equal(ctx.cur_get()[1], first[1])
    # dense after sparse
    ctx.set_v_dense(c["data"])
    assert ctx.path_name == "cur_cross_f64"
    with pytest.raises(_lib.PmfError):
        ctx.cur_get()                                          # new data: the decomposition is gone
    ctx.cur_compute(c["rid"], c["rcnt"], c["cid"], c["ccnt"])
    Cd, Ud, Rd = ctx.cur_get()
    assert cc.rel_max(Ud, c["U"]) <= c["tol_U"] and np.array_equal(Cd, first[0]) and np.array_equal(Rd, first[2])
    assert abs(ctx.frobenius() - c["ferr"]) <= (cc.FACTOR * scs.tolerances()["ferr_dense_max"]) * c["norm"]
    with pytest.raises(_lib.PmfError, match="CSR data only"):
        ctx.cur_ferr()
    ctx.cur_leverage(2, 2)                                     # the dense-only entry points are back
    # sparse after dense: the same bits as the first time
    again = run_sparse()
    for a, b in zip(first[:3], again[:3]):
        assert np.array_equal(a, b)
    assert first[3] == again[3]
    ctx.close()
