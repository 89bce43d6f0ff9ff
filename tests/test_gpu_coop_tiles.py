"""k_nmf_coop (pmf_coop.h) past one tile per workgroup: every instantiation the host reaches, at row counts where every
workgroup has a first, a middle and a last tile and some do one more (tests/coop_cases.py).

a. parity with the float64 oracle, the bars being the ones the kernel is held to at one tile per workgroup
   (test_fused8_vs_oracle, test_fused8_rnmf_free_run_and_reproducibility);
b. the W step of all rows at once equals, bit for bit, the W step of 8 192-row slices (one tile per workgroup there): the
   new W of a row depends on that row of V and W, on H and on G alone, in the same order and -- for row offsets that
   are multiples of 64 -- on the same lanes, whichever tile of whichever workgroup holds it;
c. the free-running loop equals the stepwise loop on several tiles, and two runs give identical bits.

RNMF: the single update_w hook of an RNMF context is the row GEMM, not this kernel (nmf_update_w); the kernel runs in
pmf_factorize with both updates on.  So "one step from the same state" is update_s, then ONE iteration of the loop
(update_w, update_h, the latter ending in update_s as in the reference), on both sides; every test checks through the
profiling counters that the kernel named in its id was launched as often as it thinks."""
import subprocess
import sys

import numpy as np
import pytest

import coop_cases as cc
from conftest import rel_fro, close

pytestmark = pytest.mark.gpu

CASES = cc.cases()
RAGGED = cc.ragged_cases()
NITER = 3


@pytest.fixture(scope="module")
def pm():
    import pymf_amd
    from pymf_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device: the GPU tests need an MI355X"
    return pymf_amd


@pytest.fixture(scope="module")
def cus(pm):
    """The card's CU count from torch.cuda.get_device_properties -- asked in a child process: torch ships a HIP / HSA
    runtime of its own, and a process that holds it beside the one libpymf_hip.so is linked to aborts at exit (double
    free), which is why no test imports torch beside the library (tests/_dist_worker.py)."""
    out = subprocess.run([sys.executable, "-c",
                          "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "torch" not in sys.modules
    return int(out.stdout.split()[-1])


def _require_several_tiles(m, rb, cus):
    """A differently partitioned card must fail here, not quietly test one tile per workgroup."""
    ntiles = cc.tiles(m, rb, cus)[0]
    assert ntiles >= 2 * cus + 1 and ntiles % cus != 0, (ntiles, cus)


def _launches(ctx, name):
    st = ctx.kernel_stats()
    assert st["name"] == name, st
    return st["launches"]


def _worst_tile(W, Wo, rows):
    """(worst relative Frobenius error of W over single tiles of `rows` rows, first row of that tile)."""
    d = np.einsum("ij,ij->i", W - Wo, W - Wo)
    r = np.einsum("ij,ij->i", Wo, Wo)
    at = np.arange(0, W.shape[0], rows)
    e = np.sqrt(np.add.reduceat(d, at) / np.maximum(np.add.reduceat(r, at), 1e-300))
    t = int(np.argmax(e))
    return float(e[t]), t * rows


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_coop_tiles_vs_oracle(pm, cus, cid):
    import oracle
    _, name, (bt, rb, pn), mode, kind, m, n, k = cc.case_by_id(cid)
    _require_several_tiles(m, rb, cus)
    V, W0, H0 = cc.inputs(cc.case_by_id(cid))
    cls = cc.CLASS_OF[mode]
    if mode == "rnmf":
        from pymf_amd.rnmf import RNMF
        mdl = RNMF(V, num_bases=k, lamb=cc.RNMF_LAMB)
        o = oracle.RNMFOracle(V, num_bases=k, lamb=cc.RNMF_LAMB)
    else:
        mdl = getattr(pm, cls)(V, num_bases=k)
        o = getattr(oracle, cls + "Oracle")(V, num_bases=k)
    mdl.W, mdl.H = W0.copy(), H0.copy()
    o.W, o.H = W0.copy(), H0.copy()
    mdl._context().profile_enable()
    assert mdl._ctx.path_name == name
    if mode == "rnmf":                       # one step from the same state
        mdl.update_s(); o.update_s()
        mdl.factorize(niter=1)
        o.update_w(); o.update_h()
        assert _launches(mdl._ctx, name) == 1
        w_tol, h_tol = 2e-5, 8e-7
    else:
        mdl.factorize(niter=NITER)
        o.factorize(niter=NITER)
        assert _launches(mdl._ctx, name) == NITER
        w_tol, h_tol = 2e-6, 1e-6
    W, H = np.asarray(mdl.W, dtype=np.float64), np.asarray(mdl.H, dtype=np.float64)
    ew, eh = rel_fro(W, o.W, what="mdl.W"), rel_fro(H, o.H, what="mdl.H")
    worst, row = _worst_tile(W, o.W, 16 * rb)
    b, t0, tt, ntile = cc.tile_position(row // (16 * rb), m, rb, cus)
    print("%s: W %.3g  H %.3g  worst tile W %.3g (rows %d.., workgroup %d, tile %d of %d)" % (cid, ew, eh, worst, row, b, tt, ntile))
    # (on record in the ledger, nothing asserted: there is no reference figure for a single tile yet)
    _ = rel_fro(W[row:row + 16 * rb], o.W[row:row + 16 * rb], what="worst single tile of W (reported only)") < 1.0
    assert ew < w_tol and eh < h_tol
    if mode != "rnmf":
        assert len(mdl.ferr) == len(o.ferr) == NITER
        close(mdl.ferr, o.ferr, rtol=4e-8, what="mdl.ferr")


def _w_step(_lib, mode, V, W0, H0, name, k):
    """One W step of the kernel through the C ABI on the rows given -> the new W."""
    m, n = V.shape
    ctx = _lib.Context(cc.ALGO_OF[mode], m, n, k)
    try:
        assert ctx.path_name == name
        ctx.set_v_dense(V); ctx.set_w(W0); ctx.set_h(H0)
        ctx.profile_enable()
        if mode == "bnmf":
            ctx.set_lambda(0.05, 0.05)
        if mode == "rnmf":
            # (update_w alone is the row GEMM under RNMF: the kernel's W step is the first half of an iteration, and W is
            #  not touched by the H step and the update_s behind it)
            ctx.set_lambda(0.3, 0.0)
            ctx.rnmf_update_s()
            ctx.factorize(1, compute_err=False)
        else:
            ctx.update_w()
        W = ctx.get_w()
        assert _launches(ctx, name) == 1
        return W
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", [c[0] for c in RAGGED])
def test_coop_later_tiles_equal_first_tiles_bit_for_bit(pm, cus, cid):
    from pymf_amd import _lib
    case = cc.case_by_id(cid)
    _, name, (bt, rb, pn), mode, kind, m, n, k = case
    _require_several_tiles(m, rb, cus)
    assert cc.tiles(cc.SLICE_ROWS, rb, cus)[2:] == (1, 0)          # one tile per workgroup in a slice
    V, W0, H0 = cc.inputs(case)
    W_big = _w_step(_lib, mode, V, W0, H0, name, k)
    rows = 16 * rb
    bad = []
    for r0 in range(0, m, cc.SLICE_ROWS):
        r1 = min(r0 + cc.SLICE_ROWS, m)
        W_s = _w_step(_lib, mode, V[r0:r1], W0[r0:r1], H0, name, k)
        diff = np.nonzero(np.any(W_big[r0:r1] != W_s, axis=1))[0] + r0
        bad.extend(sorted(set(int(r) // rows for r in diff)))
    if bad:
        for t in bad[:40]:
            b, t0, tt, ntile = cc.tile_position(t, m, rb, cus)
            print("tile %d (rows %d..%d) differs: workgroup %d, t0 %d, tt %d of %d" % (t, t * rows, t * rows + rows - 1, b, t0, tt, ntile))
        first = sum(1 for t in bad if cc.tile_position(t, m, rb, cus)[2] == 0)
        print("%d tiles differ: %d first tiles of their workgroup, %d later ones" % (len(bad), first, len(bad) - first))
    assert not bad, "%d tiles differ from the one-tile-per-workgroup run (first: %s)" % (len(bad), bad[:8])
    assert np.all(np.isfinite(W_big)) and np.count_nonzero(W_big) > 0.9 * W_big.size


@pytest.mark.parametrize("cid", ["k_nmf_coop<2,2,6> ragged", "k_nmf_coop<1,4,8,bnmf> ragged"])
def test_coop_free_running_loop_on_several_tiles(pm, cus, cid):
    from pymf_amd import _lib
    case = cc.case_by_id(cid)
    _, name, (bt, rb, pn), mode, kind, m, n, k = case
    _require_several_tiles(m, rb, cus)
    V, W0, H0 = cc.inputs(case)
    outs = []
    for how in ("free", "free", "step"):
        c = _lib.Context(cc.ALGO_OF[mode], m, n, k)
        try:
            assert c.path_name == name
            c.set_v_dense(V); c.set_w(W0); c.set_h(H0)
            c.profile_enable()
            if mode == "bnmf":
                c.set_lambda(1.0 / 5, 1.0 / 5)
            if how == "free":
                f, done, conv = c.factorize(5)
                assert (done, conv) == (5, -1)
                f = list(f)
            else:
                f = [c.factorize(1, conv_eps=0.0)[0][0] for _ in range(5)]
            assert _launches(c, name) == 5
            outs.append((c.get_w(), c.get_h(), np.array(f)))
        finally:
            c.close()
    for a, b_ in ((outs[0], outs[1]), (outs[0], outs[2])):
        np.testing.assert_array_equal(a[0], b_[0])
        np.testing.assert_array_equal(a[1], b_[1])
        np.testing.assert_allclose(a[2], b_[2], rtol=1e-12)
