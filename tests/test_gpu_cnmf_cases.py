"""pymf_amd.CNMF on the MI355X where tests/test_gpu_cnmf.py does not reach: every width of k_cnmf_mul_step at its lowest and
highest k, ragged k and n (the zero rows k .. KP and columns n .. np of G^T, H, L_A, L_B and S), mixed-sign data at every
width (both halves of k_cnmf_split_gemm, the P2 / L2 chain), tiny m and n, the multi-row-block chunks of the dense V^T V,
one step from a dense start, the chunk boundaries of the CNMF loop of pmf_factorize, the stop state 2 of k_conv_check, loops without the
error or without the G step, the k-means initialisation with one-member clusters, and data replaced under a live object.
The cases and their float64 oracle results: tests/cnmf_cases.py; that they leave room for float32 and reach what they are
meant for: tests/test_cnmf_cases.py.  Tolerances: DESIGN.md section 4 as in tests/test_gpu_cnmf.py -- 1e-5 relative
Frobenius on G and H, 2e-5 on W (float32), rtol 1e-5 on every ferr entry."""
import random

import numpy as np
import pytest

import cnmf_cases as cc
from conftest import close, rel_fro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pm():
    import pymf_amd
    from pymf_amd import _lib
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    return pymf_amd


def model(pm, c, H0, G0, V=None):
    mdl = pm.CNMF(cc.data(c)[0] if V is None else V, num_bases=c.k)
    mdl.H, mdl.G = np.array(H0), np.array(G0)
    return mdl


def device_run(pm, r):
    H0, G0 = cc.dense_start(r.c) if r.dense else cc.start(r.c)[:2]
    mdl = model(pm, r.c, H0, G0)
    for _ in range(r.calls):
        mdl.factorize(niter=r.niter, compute_w=r.compute_w, compute_h=r.compute_h, compute_err=r.compute_err)
    return mdl


def check(mdl, ref):
    W, H, G, ferr = ref
    assert len(mdl.ferr) == len(ferr)
    assert rel_fro(mdl.G, G, "mdl.G") < 1e-5
    assert rel_fro(mdl.H, H, "mdl.H") < 1e-5
    assert rel_fro(mdl.W, W, "mdl.W") < 2e-5
    close(mdl.ferr, ferr, rtol=1e-5, what="mdl.ferr")


# ---- 1: widths, ragged shapes, both signs -------------------------------------------------------------------------------
@pytest.mark.parametrize("r", cc.WIDTH_RUNS, ids=cc.run_id)
def test_widths_and_ragged_shapes(pm, r):
    check(device_run(pm, r), cc.run_oracle(r))


@pytest.mark.parametrize("r", cc.ONE_STEP_RUNS, ids=cc.run_id)
def test_one_step_from_a_dense_start(pm, r):
    """H only, G only, both: every entry of H0 and G0 counts, not the near-one-hot pattern of the k-means start."""
    H0, G0 = cc.dense_start(r.c)
    mdl = device_run(pm, r)
    check(mdl, cc.run_oracle(r))
    if not r.compute_w:
        assert np.array_equal(mdl.G, G0)
    if not r.compute_h:
        assert np.array_equal(mdl.H, H0)


# ---- 2: the paths of the CNMF loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", cc.LOOP_RUNS + [cc.TWICE_RUN, cc.TWICE_EARLY_RUN], ids=cc.run_id)
def test_chunk_boundaries(pm, r):
    """niter = 1, 2: by hand; 3: a chunk of two; 33, 34: a last chunk of 0 or 1 (by hand); 70: two chunks and one of five;
    two calls in a row: the second continues by hand (35 + 35) or in chunks again (8 + 8)."""
    check(device_run(pm, r), cc.run_oracle(r))


def test_loop_without_the_error(pm):
    r = cc.NO_ERR_RUN
    mdl = device_run(pm, r)
    assert np.array_equal(mdl.ferr, np.zeros(r.niter))
    W, H, G, _ = cc.run_oracle(r)
    assert rel_fro(mdl.G, G, "mdl.G") < 1e-5
    assert rel_fro(mdl.H, H, "mdl.H") < 1e-5
    assert rel_fro(mdl.W, W, "mdl.W") < 2e-5


@pytest.mark.parametrize("r", cc.NO_G_RUNS, ids=cc.run_id)
def test_loop_without_the_g_step_and_without_a_callers_w(pm, r):
    """W = V G0 throughout: G stays, so A, B, L_A and L_B are reused, not formed again or dropped."""
    mdl = device_run(pm, r)
    check(mdl, cc.run_oracle(r))
    assert np.array_equal(mdl.G, cc.start(r.c)[1])


def test_cancellation_in_the_middle_of_a_chunk(pm):
    """e^2 falls below 1e-3 tr(C) at iteration 55, inside the chunk 33 .. 64 (tests/test_cnmf_cases.py): k_conv_check raises
    stop state 2, the rest of the chunk are no-ops, the host takes the direct residual and goes on iteration by iteration."""
    r, at = cc.CANCEL_RUN, 55
    V = cc.data(r.c)[0].astype(np.float64)
    W, H, G, ferr = cc.run_oracle(r)
    mdl = device_run(pm, r)
    assert mdl._ctx.path_name == "cnmf_gram"
    assert len(mdl.ferr) == len(ferr) == cc.CANCEL_NITER
    close(mdl.ferr[:at], ferr[:at], rtol=1e-5, what="mdl.ferr from the identity")
    close(mdl.ferr[at:], ferr[at:], rtol=1e-5, what="mdl.ferr from the direct residual")
    assert rel_fro(mdl.G, G, "mdl.G") < 1e-5
    assert rel_fro(mdl.H, H, "mdl.H") < 1e-5
    assert rel_fro(mdl.W, W, "mdl.W") < 2e-5
    close(mdl.frobenius_norm(), np.sqrt(np.sum((V - W.dot(H)) ** 2)), rtol=1e-5, what="mdl.frobenius_norm()")


# ---- 3: the k-means initialisation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.INIT_CASES, ids=cc.case_id)
def test_kmeans_initialisation(pm, c):
    """As test_initialisation_matches_reference: the same clusters, H bit for bit, G to 1e-14 -- with one-member clusters
    (k_kmeans_update leaves their centres), n == k, m < 16, and the assigned array of the C ABI."""
    from pymf_amd import _lib
    V, sel, labels = cc.data(c)
    H0, G0, assigned, gap = cc.start(c)
    assert np.array_equal(assigned, labels) and gap >= 1e-2
    random.seed(c.seed)
    mdl = pm.CNMF(V, num_bases=c.k)
    mdl.factorize(niter=0)
    assert len(mdl.ferr) == 0
    assert np.array_equal(np.argmax(mdl.H, axis=0), labels)
    assert np.array_equal(mdl.H, H0)
    assert rel_fro(mdl.G, G0, "mdl.G") < 1e-14
    assert rel_fro(mdl.W, V.astype(np.float64).dot(G0), "mdl.W") < 2e-5
    ctx = _lib.Context(_lib.ALGO_CNMF, c.m, c.n, c.k)
    try:
        ctx.set_v_dense(V)
        assert np.array_equal(ctx.cnmf_init(sel), labels)
        assert np.array_equal(ctx.get_h64(), H0)
    finally:
        ctx.close()


# ---- 4: fixed order, state that follows the data ------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(pm):
    """Every sum in pmf_cnmf.h has a fixed order."""
    r = cc.run(cc.Case(70, 200, 33, cc.SEED, 0.05, 0.5), 40)
    assert r in cc.WIDTH_RUNS
    runs = []
    for _ in range(2):
        mdl = device_run(pm, r)
        runs.append((mdl.G.copy(), mdl.H.copy(), mdl.W.copy(), mdl.ferr.copy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_replaced_data_of_another_sign_pattern_are_followed(pm):
    """data of shift 0, then of shift 0.5 under the same object: C, its trace, A, B and L are all formed again."""
    a, b = cc.REPLACE_FROM, cc.REPLACE_TO
    mdl = model(pm, a, *cc.start(a)[:2])
    mdl.factorize(niter=cc.REPLACE_NITER)
    check(mdl, cc.run_oracle(cc.run(a, cc.REPLACE_NITER)))
    mdl.data = cc.data(b)[0]
    mdl.factorize(niter=cc.REPLACE_NITER)
    check(mdl, cc.replaced_oracle())
