"""The cases of tests/nmf_sparse_cases.py leave room for float32 and reach what they are meant for (no GPU): a failure of
tests/test_gpu_nmf_sparse.py on the device is then the kernel's, not the case's.  (a) The gather-form update restated in
float32 NumPy -- the arithmetic of k_nmf_sp_step whatever its summation order -- stays within a quarter of the device
tolerance of the float64 oracle on every run the device test compares.  (b) The corner matrix has the rows, columns and
stored entries its name promises.  (c) The shapes reach every kernel width at both ends, one and several workgroups."""
import numpy as np
import pytest

pytest.importorskip("scipy.sparse")
import nmf_sparse_cases as nc  # noqa: E402


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))


def room(tag, c, **kw):
    W, H = nc.oracle_run(c, **kw)
    W32, H32 = nc.gather32(c, **kw)
    got = {"W": rel(W32, W), "H": rel(H32, H)}
    print(tag, {q: "%.2g of %.2g" % (v, nc.TOL / 4) for q, v in got.items()})
    assert np.isfinite(W).all() and np.isfinite(H).all() and W.min() >= 0.0 and H.min() >= 0.0
    for q, v in got.items():
        assert v <= nc.TOL / 4, (q, v)


# ---- (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nc.WIDTH_CASES + [nc.CORNER, nc.ABI_CASE], ids=nc.case_id)
def test_case_leaves_room_for_float32(c):
    room(nc.case_id(c), c)


@pytest.mark.parametrize("kw", [dict(niter=nc.LOOP_NITER), dict(compute_w=False), dict(compute_h=False)],
                         ids=["niter6", "noW", "noH"])
def test_loop_runs_leave_room_for_float32(kw):
    room("loop case %r" % (kw,), nc.LOOP_CASE, **kw)


def test_golden_cases_leave_room_for_float32():
    """The two goldens (tests/golden/gen_golden_nmf_sparse.py: the reference's own W and H): the same restatement on them."""
    import os
    import sys
    import scipy.sparse as sp
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_golden_nmf_sparse as gg
    for name, (m, n, k, density, niter, seed) in gg.CASES.items():
        g = dict(np.load(os.path.join(os.path.dirname(gg.__file__), name + ".npz")))
        if "W" not in g:
            g.update(np.load(os.path.join(os.path.dirname(gg.__file__), name + "_w.npz")))
        V = sp.csr_matrix((g["data"].astype(np.float64), g["indices"], g["indptr"]), shape=(m, n))
        assert (V != gg.matrix(m, n, density, seed)).nnz == 0 and int(g["niter"]) == niter and int(g["k"]) == k
        W0, H0 = gg.start(m, n, k, seed)
        W, Ht = W0.astype(np.float32), np.ascontiguousarray(H0.T.astype(np.float32))
        V32, eps = V.astype(np.float32), np.float32(1e-9)
        Vt32 = V32.T.tocsr()
        G = Ht.T.dot(Ht)
        for _ in range(niter):
            W = (W * V32.dot(Ht)) / (W.dot(G) + eps)
            G = W.T.dot(W)
            Ht = (Ht * Vt32.dot(W)) / (Ht.dot(G) + eps)
            G = Ht.T.dot(Ht)
        got = (rel(W, g["W"]), rel(Ht.T, g["H"]))
        print(name, "W %.2g H %.2g of %.2g" % (got + (nc.TOL / 4,)))
        assert max(got) <= nc.TOL / 4


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def test_the_corner_matrix_has_its_corners():
    f = nc.corner_formats()
    can, raw = f["canonical"], f["raw_csr"]
    assert can.has_canonical_format and not raw.has_canonical_format
    counts = np.diff(can.indptr)
    for r in nc.CORNER_EMPTY_ROWS:
        assert counts[r] == 0
    for r, cnt in nc.CORNER_LONG_ROWS.items():
        assert counts[r] == cnt and r // 16 == 0                      # one 16-row block: entries 0 .. 491 of it
    col_counts = np.bincount(can.indices, minlength=nc.CORNER.n)
    assert all(col_counts[q] == 0 for q in nc.CORNER_EMPTY_COLS) and np.sum(col_counts == 0) == len(nc.CORNER_EMPTY_COLS)
    assert np.sum(can.data == 0.0) > 50                               # stored explicit zeros survive sum_duplicates
    assert raw.nnz > can.nnz + 100                                    # unsummed duplicates
    dense = can.toarray()
    for name in ("raw_csr", "coo", "csc"):
        assert np.array_equal(f[name].toarray(), dense), name
    assert f["coo"].format == "coo" and f["csc"].format == "csc"
    assert float(dense.min()) >= 0.0
    assert np.array_equal(dense.astype(np.float32).astype(np.float64), dense)


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_the_ranges_they_are_meant_for():
    ks = {}
    for c in nc.WIDTH_CASES:
        ks.setdefault(nc.geometry(c.m, c.n, c.k)["NT"], set()).add(c.k)
    assert {nt: (min(v), max(v)) for nt, v in ks.items()} == {1: (1, 16), 2: (17, 32), 4: (33, 64), 8: (65, 128)}
    g = {(c.m, c.n): nc.geometry(c.m, c.n, 128) for c in nc.WIDTH_CASES}
    assert g[(37, 29)]["wgs_w"] == 1 and g[(37, 29)]["wgs_h"] == 1
    assert g[(1003, 520)]["wgs_w"] == 16 and g[(1003, 520)]["wgs_h"] == 9
    assert g[(5000, 300)]["wgs_w"] == 79                              # several workgroups: the slab sum adds 79 slabs
    # n = 520 with 100 bases: np * KP * 4 bytes is beyond the 160 KiB at which the SNMF CSR path expands the rows
    a = nc.geometry(nc.ABI_CASE.m, nc.ABI_CASE.n, nc.ABI_CASE.k)
    assert a["np"] * a["KP"] * 4 > 160 * 1024
    # every value is float32-representable and the matrices are as sparse as they say
    for c in (nc.WIDTH_CASES[0], nc.LOOP_CASE, nc.WIDTH_CASES[-1]):
        V = nc.matrix(c)
        assert np.array_equal(V.data.astype(np.float32).astype(np.float64), V.data)
        assert abs(V.nnz / float(c.m * c.n) - c.density) < 0.1 * c.density + 1e-3
