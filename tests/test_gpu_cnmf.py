"""pymf_amd.CNMF on the MI355X against the reference's own results (tests/golden/cnmf_*.npz) and the float64 NumPy oracle
(tests/cnmf_oracle.py).  Tolerances: C = V^T V carries about 1e-7 relative error (fp32 products, float64 sums), G and H
are float64 on the device; W = V G is float32."""
import glob
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, close, load_golden, rel_fro
import cnmf_oracle
from cnmf_cases import planted as _planted

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "cnmf_*.npz")))
INIT_CASES = [c for c in CASES if int(np.load(os.path.join(GOLDEN, c + ".npz"))["niter"]) == 0]
ITER_CASES = [c for c in CASES if c not in INIT_CASES]


@pytest.fixture(scope="module")
def pm():
    import pymf_amd
    from pymf_amd import _lib
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    return pymf_amd


def _run_golden(pm, d):
    V = d["V"]
    random.seed(int(d["random_seed"]))
    mdl = pm.CNMF(V, num_bases=int(d["k"]))
    if "W_user" in d:
        mdl.W = d["W_user"].copy()
    mdl.factorize(niter=int(d["niter"]), compute_w=bool(d["compute_w"]), compute_h=bool(d["compute_h"]))
    return mdl


@pytest.mark.parametrize("name", INIT_CASES)
def test_initialisation_matches_reference(pm, name):
    """k-means + init_h (cnmf.py:78-103): the same clusters, H bit for bit, G to 1e-14."""
    d = load_golden(name)
    mdl = _run_golden(pm, d)
    assert len(mdl.ferr) == 0
    assert np.array_equal(np.argmax(mdl.H, axis=0), np.argmax(d["H"], axis=0))
    assert np.array_equal(mdl.H, d["H"])
    assert rel_fro(mdl.G, d["G"], "mdl.G") < 1e-14
    assert rel_fro(mdl.W, d["W"], "mdl.W") < 2e-5


@pytest.mark.parametrize("name", ITER_CASES)
def test_factorize_matches_reference_golden(pm, name):
    d = load_golden(name)
    mdl = _run_golden(pm, d)
    assert len(mdl.ferr) == len(d["ferr"])
    assert rel_fro(mdl.G, d["G"], "mdl.G") < 1e-5
    assert rel_fro(mdl.H, d["H"], "mdl.H") < 1e-5
    Wref = d["W"] if "W" in d else d["V"].astype(np.float64).dot(d["G"])
    assert rel_fro(mdl.W, Wref, "mdl.W") < 2e-5
    close(mdl.ferr, d["ferr"], rtol=1e-5, what="mdl.ferr")


@pytest.mark.parametrize("m,n,k,niter", [(262144, 256, 32, 10), (4096, 1024, 128, 10)])
def test_planted_clusters_vs_oracle(pm, m, n, k, niter):
    V, sel, labels = _planted(m, n, k, 1234)
    Vd = V.astype(np.float64)
    H0, G0, assigned = cnmf_oracle.cnmf_init(Vd, k, sel, vq_fn=cnmf_oracle.vq_gram)
    assert np.array_equal(assigned, labels)
    W, H, G, ferr = cnmf_oracle.cnmf_factorize(Vd, H0, G0, niter=niter)
    random.seed(1234)
    mdl = pm.CNMF(V, num_bases=k)
    mdl.factorize(niter=niter)
    assert np.array_equal(np.argmax(mdl.H, axis=0), np.argmax(H, axis=0))
    assert len(mdl.ferr) == len(ferr)
    assert rel_fro(mdl.G, G, "mdl.G") < 1e-5
    assert rel_fro(mdl.H, H, "mdl.H") < 1e-5
    assert rel_fro(mdl.W, W, "mdl.W") < 2e-5
    close(mdl.ferr, ferr, rtol=1e-5, what="mdl.ferr")


def test_float64_h_and_g_round_trip_exactly(pm):
    from pymf_amd import _lib
    n, k = 200, 12
    ctx = _lib.Context(_lib.ALGO_CNMF, 96, n, k)
    rs = np.random.RandomState(3)
    H = rs.random_sample((k, n)) + 1e-17
    G = rs.random_sample((n, k)) / 3.0
    ctx.set_h(H)
    ctx.set_g(G)
    assert np.array_equal(ctx.get_h64(), H)
    assert np.array_equal(ctx.get_g(), G)
    ctx.close()


def test_a_filled_w_is_the_w_that_is_read_back(pm):
    """pmf_set_g_f64 binds W = V G (materialised when it is read); pmf_fill_w_uniform behind it replaces W like
    pmf_set_w_* does: the W read back is the fill, bit for bit, not V G written over it."""
    from pymf_amd import _lib
    m, n, k = 96, 200, 12
    rs = np.random.RandomState(4)
    ctx = _lib.Context(_lib.ALGO_CNMF, m, n, k)
    ctx.set_v_dense(rs.random_sample((m, n)).astype(np.float32))
    ctx.set_g(rs.random_sample((n, k)) / 3.0)
    ctx.fill_w_uniform(7)
    W = ctx.get_w()
    ctx.close()
    ref = _lib.Context(_lib.ALGO_NMF, m, n, k)
    ref.fill_w_uniform(7)
    assert np.array_equal(W, ref.get_w())
    ref.close()


def _golden_state(name="cnmf_300x64_k6"):
    d = load_golden(name)
    V = d["V"].astype(np.float64)
    random.seed(int(d["random_seed"]))
    sel = np.sort(random.sample(range(V.shape[1]), int(d["k"])))
    H0, G0, _ = cnmf_oracle.cnmf_init(V, int(d["k"]), sel)
    return d, H0, G0


def test_second_factorize_continues_from_the_first(pm):
    d, H0, G0 = _golden_state()
    V = d["V"]
    mdl = pm.CNMF(V, num_bases=int(d["k"]))
    mdl.H, mdl.G = H0.copy(), G0.copy()
    mdl.factorize(niter=4)
    mdl.factorize(niter=6)
    W1, H1, G1, _ = cnmf_oracle.cnmf_factorize(V, H0, G0, niter=4)
    W2, H2, G2, ferr2 = cnmf_oracle.cnmf_factorize(V, H1, G1, niter=6)
    assert rel_fro(mdl.G, G2, "mdl.G") < 1e-5
    assert rel_fro(mdl.H, H2, "mdl.H") < 1e-5
    close(mdl.ferr, ferr2, rtol=1e-5, what="mdl.ferr")


def test_in_place_edit_of_data_is_seen(pm):
    d, H0, G0 = _golden_state()
    V = d["V"].copy()
    mdl = pm.CNMF(V, num_bases=int(d["k"]))
    mdl.H, mdl.G = H0.copy(), G0.copy()
    mdl.factorize(niter=3)
    V[:, 5] *= np.float32(1.5)                      # same object, new bytes: C must be formed again
    V[7, :] += np.float32(0.25)
    mdl.factorize(niter=3)
    _, H1, G1, _ = cnmf_oracle.cnmf_factorize(d["V"], H0, G0, niter=3)
    _, H2, G2, ferr2 = cnmf_oracle.cnmf_factorize(V, H1, G1, niter=3)
    assert rel_fro(mdl.G, G2, "mdl.G") < 1e-5
    assert rel_fro(mdl.H, H2, "mdl.H") < 1e-5
    close(mdl.ferr, ferr2, rtol=1e-5, what="mdl.ferr")


def test_user_w_is_what_the_error_uses(pm):
    d, H0, G0 = _golden_state()
    V = d["V"]
    Wu = np.random.RandomState(9).random_sample((V.shape[0], int(d["k"])))
    mdl = pm.CNMF(V, num_bases=int(d["k"]))
    mdl.H, mdl.G, mdl.W = H0.copy(), G0.copy(), Wu.copy()
    mdl.factorize(niter=5, compute_w=False)
    _, H, G, ferr = cnmf_oracle.cnmf_factorize(V, H0, G0, W=Wu, niter=5, compute_w=False)
    assert np.array_equal(mdl.W, Wu)
    assert rel_fro(mdl.H, H, "mdl.H") < 1e-5
    close(mdl.ferr, ferr, rtol=1e-5, what="mdl.ferr")
    close(mdl.frobenius_norm(), np.sqrt(np.sum((V - Wu.dot(H)) ** 2)), rtol=1e-5, what="mdl.frobenius_norm()")


def test_overridden_frobenius_norm_is_called_every_iteration(pm):
    d, H0, G0 = _golden_state()

    class Counting(pm.CNMF):
        calls = 0

        def frobenius_norm(self):
            Counting.calls += 1
            return pm.CNMF.frobenius_norm(self)

    mdl = Counting(d["V"], num_bases=int(d["k"]))
    mdl.H, mdl.G = H0.copy(), G0.copy()
    mdl.factorize(niter=5)
    assert Counting.calls == 5
    _, H, G, ferr = cnmf_oracle.cnmf_factorize(d["V"], H0, G0, niter=5)
    assert rel_fro(mdl.G, G, "mdl.G") < 1e-5
    assert rel_fro(mdl.H, H, "mdl.H") < 1e-5
    close(mdl.ferr, ferr, rtol=1e-5, what="mdl.ferr")
