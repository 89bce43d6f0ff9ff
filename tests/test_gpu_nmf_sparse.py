"""pymf_amd.NMF on scipy.sparse data (accept_sparse = True) on the MI355X: k_nmf_sp_step (pmf_nmf_csr.h) against the
reference's own results on toarray() (tests/golden/nmfsp_*.npz, gen_golden_nmf_sparse.py) and against the float64 oracle
over the kernel's corners (tests/nmf_sparse_cases.py; that the cases leave room for float32: tests/test_nmf_sparse_cases.py).
Tolerance: DESIGN.md section 4, NMF -- 2e-5 relative Frobenius on W and on H."""
import os

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
import nmf_sparse_cases as nc  # noqa: E402
from conftest import GOLDEN, rel_fro  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = nc.TOL


@pytest.fixture(scope="module")
def pm():
    import pymf_amd
    from pymf_amd import _lib
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    return pymf_amd


def model(pm, c, V=None, cls=None):
    W0, H0 = nc.start(c)
    mdl = (cls or pm.NMF)(nc.matrix(c).astype(np.float32) if V is None else V, num_bases=c.k)
    mdl.accept_sparse = True
    mdl.W, mdl.H = W0.copy(), H0.copy()
    return mdl


def check(mdl, ref, tag=""):
    W, H = ref
    assert rel_fro(mdl.W, W, tag + "W") < TOL
    assert rel_fro(mdl.H, H, tag + "H") < TOL


# ---- 1: the reference's own numbers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nmfsp_300x200_k6", "nmfsp_1000x520_k100"])
def test_goldens(pm, name):
    import sys
    sys.path.insert(0, GOLDEN)
    import gen_golden_nmf_sparse as gg
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "W" not in g:
        g.update(np.load(os.path.join(GOLDEN, name + "_w.npz")))
    m, n = (int(x) for x in g["shape"])
    k = int(g["k"])
    V = sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(m, n))
    W0, H0 = gg.start(m, n, k, int(g["seed"]))
    mdl = pm.NMF(V, num_bases=k)
    mdl.accept_sparse = True
    mdl.W, mdl.H = W0.copy(), H0.copy()
    mdl.factorize(niter=int(g["niter"]), compute_err=False)
    assert mdl._ctx.path_name.startswith("nmf_csr_gather")
    assert rel_fro(mdl.W, g["W"], "W vs pymf.NMF on toarray()") < TOL
    assert rel_fro(mdl.H, g["H"], "H vs pymf.NMF on toarray()") < TOL
    assert mdl.frobenius_norm() == -123456


# ---- 2: oracle parity over the kernel's corners ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", nc.WIDTH_CASES, ids=nc.case_id)
def test_widths_and_shapes(pm, c):
    mdl = model(pm, c)
    mdl.factorize(niter=nc.NITER, compute_err=False)
    check(mdl, nc.oracle_run(c))
    W, H = mdl.W, mdl.H
    assert np.isfinite(W).all() and np.isfinite(H).all() and W.min() >= 0.0 and H.min() >= 0.0


@pytest.mark.parametrize("fmt", ["canonical", "raw_csr", "coo", "csc"])
def test_corner_matrix_in_every_format(pm, fmt):
    """Empty rows and columns, rows of 63, 64, 65 and 300 entries in one block, stored zeros, unsummed duplicates."""
    c = nc.CORNER
    V = nc.corner_formats()[fmt].astype(np.float32)
    mdl = model(pm, c, V=V)
    mdl.factorize(niter=nc.NITER, compute_err=False)
    check(mdl, nc.oracle_run(c), fmt + ": ")
    W, H = mdl.W, mdl.H
    assert not W[list(nc.CORNER_EMPTY_ROWS)].any()             # W *= 0, as in the reference
    assert not H[:, list(nc.CORNER_EMPTY_COLS)].any()
    assert (W[[3, 4, 5, 6]] > 0).all()


# ---- 3: the forms of the loop ------------------------------------------------------------------------------------------
def test_loop_forms_agree_bit_for_bit(pm):
    c = nc.LOOP_CASE
    one = model(pm, c)
    one.factorize(niter=nc.LOOP_NITER, compute_err=False)
    check(one, nc.oracle_run(c, niter=nc.LOOP_NITER), "factorize(6): ")

    twice = model(pm, c)
    twice.factorize(niter=3, compute_err=False)
    twice.factorize(niter=3, compute_err=False)

    hand = model(pm, c)
    for _ in range(2):
        for _ in range(3):
            hand.update_w()
            hand.update_h()

    class Mine(pm.NMF):
        calls = 0

        def update_h(self):
            type(self).calls += 1
            pm.NMF.update_h(self)

    hooks = model(pm, c, cls=Mine)
    hooks.factorize(niter=nc.LOOP_NITER, compute_err=False)
    assert Mine.calls == nc.LOOP_NITER
    for tag, other in (("factorize(3) twice", twice), ("by hand", hand), ("subclass hooks", hooks)):
        assert np.array_equal(other.W, one.W), tag
        assert np.array_equal(other.H, one.H), tag


@pytest.mark.parametrize("cw,ch", [(False, True), (True, False)], ids=["noW", "noH"])
def test_one_factor_fixed(pm, cw, ch):
    c = nc.LOOP_CASE
    W0, H0 = nc.start(c)
    mdl = model(pm, c)
    mdl.factorize(niter=nc.NITER, compute_w=cw, compute_h=ch, compute_err=False)
    check(mdl, nc.oracle_run(c, compute_w=cw, compute_h=ch))
    if not cw:
        assert np.array_equal(mdl.W, W0)
    if not ch:
        assert np.array_equal(mdl.H, H0)
    # ... and the factor left alone and its Gram matrix are still good for a full iteration
    mdl.factorize(niter=1, compute_err=False)
    o = __import__("oracle").NMFOracle(nc.matrix(c).toarray(), num_bases=c.k)
    o.W, o.H = (np.array(x) for x in nc.oracle_run(c, compute_w=cw, compute_h=ch))
    o.factorize(niter=1, compute_err=False)
    check(mdl, (o.W, o.H), "one more iteration: ")


# ---- 4: reproducible ----------------------------------------------------------------------------------------------------
def test_two_fresh_objects_give_the_same_bits(pm):
    c = nc.WIDTH_CASES[-1]                                     # 5000 x 300, k = 128: 79 workgroups in the W step
    a, b = model(pm, c), model(pm, c)
    a.factorize(niter=nc.NITER, compute_err=False)
    b.factorize(niter=nc.NITER, compute_err=False)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H)


# ---- 5: data handling ---------------------------------------------------------------------------------------------------
def test_replaced_data_are_uploaded_again(pm):
    c, c2 = nc.LOOP_CASE, nc.LOOP_CASE._replace(seed=8)
    mdl = model(pm, c)
    mdl.factorize(niter=nc.NITER, compute_err=False)
    check(mdl, nc.oracle_run(c))
    mdl.data = nc.matrix(c2).astype(np.float32)
    mdl.factorize(niter=nc.NITER, compute_err=False)
    o = __import__("oracle").NMFOracle(nc.matrix(c2).toarray(), num_bases=c.k)
    o.W, o.H = (np.array(x) for x in nc.oracle_run(c))
    o.factorize(niter=nc.NITER, compute_err=False)
    check(mdl, (o.W, o.H), "second matrix: ")


def test_an_edit_in_place_is_noticed_under_check_data(pm):
    c = nc.LOOP_CASE
    V = nc.matrix(c).astype(np.float32)
    mdl = model(pm, c, V=V)
    assert mdl.check_data
    mdl.factorize(niter=1, compute_err=False)
    V.data[::2] *= 2.0                                         # (exact in float32)
    mdl.factorize(niter=2, compute_err=False)
    o = __import__("oracle").NMFOracle(nc.matrix(c).toarray(), num_bases=c.k)
    W0, H0 = nc.start(c)
    o.W, o.H = W0.copy(), H0.copy()
    o.factorize(niter=1, compute_err=False)
    o.data = V.toarray().astype(np.float64)
    o.factorize(niter=2, compute_err=False)
    check(mdl, (o.W, o.H), "edited data: ")


def test_no_dense_v_on_the_device(pm):
    """1003 x 520 with 100 bases: where an SNMF context expands the rows (np KP 4 bytes > 160 KiB), the NMF context keeps CSR."""
    from pymf_amd import _lib
    c = nc.ABI_CASE
    V = nc.matrix(c)
    ctx = _lib.Context(_lib.ALGO_NMF, c.m, c.n, c.k)
    try:
        dense_path = ctx.path_name
        ctx.set_v_csr(V.indptr, V.indices, V.data)
        assert ctx.path_name == "nmf_csr_gather<8>" and dense_path != ctx.path_name
        ctx.set_v_dense(V.toarray().astype(np.float32))        # dense data again: the dense path's name again
        assert ctx.path_name == dense_path
        ctx.set_v_csr(V.indptr, V.indices, V.data)
        assert ctx.path_name == "nmf_csr_gather<8>"
    finally:
        ctx.close()


# ---- 6: the C ABI alone ---------------------------------------------------------------------------------------------------
def test_c_abi_alone(pm):
    from pymf_amd import _lib
    c = nc.ABI_CASE
    V = nc.matrix(c)
    W0, H0 = nc.start(c)
    ctx = _lib.Context(_lib.ALGO_NMF, c.m, c.n, c.k)
    try:
        ctx.set_v_csr(V.indptr, V.indices, V.data)
        ctx.set_w(W0.astype(np.float32)); ctx.set_h(H0.astype(np.float32))
        for _ in range(nc.NITER):
            ctx.update_w()
            ctx.update_h()
        W, H = ctx.get_w(), ctx.get_h()
        with pytest.raises(_lib.PmfError, match="frobenius on CSR data") as e:
            ctx.frobenius()
        assert e.value.code == _lib.PMF_EINVAL
    finally:
        ctx.close()
    Wo, Ho = nc.oracle_run(c)
    assert rel_fro(W, Wo, "C ABI W") < TOL
    assert rel_fro(H, Ho, "C ABI H") < TOL


def test_c_abi_takes_unsummed_duplicates(pm):
    from pymf_amd import _lib
    c = nc.CORNER
    raw = nc.corner_formats()["raw_csr"]
    W0, H0 = nc.start(c)
    ctx = _lib.Context(_lib.ALGO_NMF, c.m, c.n, c.k)
    try:
        ctx.set_v_csr(raw.indptr, raw.indices, raw.data)
        ctx.set_w(W0.astype(np.float32)); ctx.set_h(H0.astype(np.float32))
        ferr, done, conv = ctx.factorize(nc.NITER, compute_err=False)
        assert done == nc.NITER
        W, H = ctx.get_w(), ctx.get_h()
    finally:
        ctx.close()
    Wo, Ho = nc.oracle_run(c)
    assert rel_fro(W, Wo, "C ABI W, duplicates") < TOL
    assert rel_fro(H, Ho, "C ABI H, duplicates") < TOL


def test_c_abi_limits(pm):
    from pymf_amd import _lib
    V = nc.matrix(nc.ABI_CASE)
    ctx = _lib.Context(_lib.ALGO_NMF, nc.ABI_CASE.m, nc.ABI_CASE.n, 129)
    try:
        with pytest.raises(_lib.PmfError, match="num_bases > 128") as e:
            ctx.set_v_csr(V.indptr, V.indices, V.data)
        assert e.value.code == _lib.PMF_EINVAL
    finally:
        ctx.close()
    # more than one rank: a context whose sums cross ranks (here through the host transport; a two-rank RCCL communicator
    # cannot be formed inside one process) refuses the upload -- and a step, if the transport arrives after the upload
    ctx = _lib.Context(_lib.ALGO_NMF, nc.ABI_CASE.m, nc.ABI_CASE.n, 8)
    try:
        ctx.set_host_allreduce(lambda a: a)
        with pytest.raises(_lib.PmfError, match="one rank only") as e:
            ctx.set_v_csr(V.indptr, V.indices, V.data)
        assert e.value.code == _lib.PMF_EINVAL
    finally:
        ctx.close()
    ctx = _lib.Context(_lib.ALGO_NMF, nc.ABI_CASE.m, nc.ABI_CASE.n, 8)
    try:
        ctx.set_v_csr(V.indptr, V.indices, V.data)
        ctx.fill_w_uniform(1); ctx.fill_h_uniform(2)
        ctx.set_host_allreduce(lambda a: a)
        with pytest.raises(_lib.PmfError, match="one rank only") as e:
            ctx.update_w()
        assert e.value.code == _lib.PMF_EINVAL
    finally:
        ctx.close()
    # every other family but SNMF keeps the present refusal
    for algo in (_lib.ALGO_BNMF, _lib.ALGO_NMFALS):
        ctx = _lib.Context(algo, nc.ABI_CASE.m, nc.ABI_CASE.n, 8)
        try:
            with pytest.raises(_lib.PmfError, match="CSR input is only wired for") as e:
                ctx.set_v_csr(V.indptr, V.indices, V.data)
            assert e.value.code == _lib.PMF_EINVAL
        finally:
            ctx.close()
    # a column index beyond n and a decreasing row pointer are refused on the host, before anything is uploaded
    ctx = _lib.Context(_lib.ALGO_NMF, 4, 5, 2)
    try:
        with pytest.raises(_lib.PmfError, match="column index out of range"):
            ctx.set_v_csr(np.array([0, 1, 1, 1, 2]), np.array([1, 5]), np.array([1.0, 1.0]))
        with pytest.raises(_lib.PmfError, match="indptr"):
            ctx.set_v_csr(np.array([0, 2, 1, 1, 2]), np.array([1, 2]), np.array([1.0, 1.0]))
    finally:
        ctx.close()
