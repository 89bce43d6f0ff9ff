"""pymf_amd.Kmeans / pymf_amd.Cmeans on the MI355X against the reference goldens and the float64 oracle
(tests/cluster_oracle.py).  Trajectories are compared only where the reference's own near-ties leave room for float32
(goldens with a recorded gap >= 1e-4 of ||v||, planted clusters started from perturbed true centres); on unstructured data at
large n the properties of every iteration are checked instead.  Tolerance: DESIGN.md section 4, 2e-5 relative Frobenius."""
import functools
import random

import numpy as np
import pytest

import cluster_oracle as co
import pymf_amd
from cluster_cases import CMEANS_GOLDENS, KMEANS_GOLDENS, load_case, onehot
from conftest import close, rel_fro

pytestmark = pytest.mark.gpu

TOL = 2e-5
BLOB_CASES = [(64, 5000, 8), (130, 4500, 33), (37, 4100, 5)]     # several 64-column panels, a ragged last one


@functools.lru_cache(maxsize=None)
def blob_data(m, n, k, seed=300):
    V, W0, _ = co.blobs(m, n, k, seed + m)
    V.setflags(write=False)
    W0.setflags(write=False)
    return V, W0


@functools.lru_cache(maxsize=None)
def kmeans_oracle(m, n, k, niter=6):
    V, W0 = blob_data(m, n, k)
    out = co.kmeans(V, k, W=W0, niter=niter)
    assert out[4] >= 1e-4, "the case itself has a near-tie: %g" % out[4]
    return out


@functools.lru_cache(maxsize=None)
def cmeans_oracle(m, n, k, niter=4):
    V, W0 = blob_data(m, n, k)
    H0 = np.random.RandomState(7).random_sample((k, n))
    return (H0,) + tuple(co.cmeans(V, W0, H0, niter=niter))


def device_kmeans(V, k, W0=None, cls=None, **kw):
    mdl = (cls or pymf_amd.Kmeans)(V, num_bases=k)
    if W0 is not None:
        mdl.W = np.array(W0)
    mdl.factorize(**kw)
    return mdl


def check_kmeans(mdl, W, H, assigned, ferr, tag):
    assert np.array_equal(mdl.assigned, assigned), "%s: %d samples assigned differently" % (
        tag, int(np.sum(np.asarray(mdl.assigned) != assigned)))
    assert np.array_equal(mdl.H, H)
    assert rel_fro(mdl.W, W, tag + " W") < TOL
    if ferr is not None:
        assert len(mdl.ferr) == len(ferr)
        close(mdl.ferr, ferr, rtol=TOL, what=tag + " ferr")


# ---- 1, 2: the reference's goldens ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KMEANS_GOLDENS)
def test_kmeans_golden(name):
    g = load_case(name)
    k, ce = int(g["k"]), bool(g["compute_err"])
    random.seed(int(g["random_seed"]))
    mdl = device_kmeans(g["V"], k, niter=int(g["niter"]), compute_err=ce)
    check_kmeans(mdl, g["W"], onehot(g["assigned"], k), g["assigned"], g["ferr"] if ce else None, name)


@pytest.mark.parametrize("name", CMEANS_GOLDENS)
def test_cmeans_golden(name):
    g = load_case(name)
    np.random.seed(int(g["np_seed"]))
    mdl = pymf_amd.Cmeans(g["V"], num_bases=int(g["k"]))
    if "W_user" in g:
        mdl.W = g["W_user"].copy()
    mdl.factorize(niter=int(g["niter"]), compute_w=bool(g["compute_w"]))
    assert len(mdl.ferr) == len(g["ferr"])
    assert rel_fro(mdl.W, g["W"], name + " W") < TOL
    assert rel_fro(mdl.H, g["H"], name + " H") < TOL
    close(mdl.ferr, g["ferr"], rtol=TOL, what=name + " ferr")


# ---- 3: large n from perturbed true centres: the column-panel path ---------------------------------------------------------
@pytest.mark.parametrize("m,n,k", BLOB_CASES)
def test_kmeans_large_n(m, n, k):
    V, W0 = blob_data(m, n, k)
    W, H, assigned, ferr, gap = kmeans_oracle(m, n, k)
    mdl = device_kmeans(V, k, W0, niter=6)
    check_kmeans(mdl, W, H, assigned, ferr, "kmeans %dx%d k%d" % (m, n, k))


@pytest.mark.parametrize("m,n,k", BLOB_CASES)
def test_cmeans_large_n(m, n, k):
    V, W0 = blob_data(m, n, k)
    H0, W, H, ferr = cmeans_oracle(m, n, k)
    mdl = pymf_amd.Cmeans(V, num_bases=k)
    mdl.W, mdl.H = np.array(W0), H0.copy()
    mdl.factorize(niter=4)
    tag = "cmeans %dx%d k%d" % (m, n, k)
    assert len(mdl.ferr) == len(ferr)
    assert rel_fro(mdl.W, W, tag + " W") < TOL
    assert rel_fro(mdl.H, H, tag + " H") < TOL
    close(mdl.ferr, ferr, rtol=TOL, what=tag + " ferr")


# ---- 4: kernel widths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16, 17, 64, 128])
def test_kernel_widths(k):
    V, W0 = blob_data(48, 600, k)
    W, H, assigned, ferr, gap = co.kmeans(V, k, W=W0, niter=3)
    assert k == 1 or gap >= 1e-4
    check_kmeans(device_kmeans(V, k, W0, niter=3), W, H, assigned, ferr, "kmeans width %d" % k)
    H0 = np.random.RandomState(k).random_sample((k, 600))
    Wc, Hc, fc = co.cmeans(V, W0, H0, niter=3)
    mdl = pymf_amd.Cmeans(V, num_bases=k)
    mdl.W, mdl.H = np.array(W0), H0.copy()
    mdl.factorize(niter=3)
    assert rel_fro(mdl.W, Wc, "cmeans width %d W" % k) < TOL
    assert rel_fro(mdl.H, Hc, "cmeans width %d H" % k) < TOL
    close(mdl.ferr, fc, rtol=TOL, what="cmeans width %d ferr" % k)


@pytest.mark.parametrize("cls", ["Kmeans", "Cmeans"])
def test_129_bases_are_refused(cls):
    with pytest.raises(ValueError):
        getattr(pymf_amd, cls)(blob_data(48, 600, 16)[0], num_bases=129).factorize(niter=1)


# ---- 5: rows beyond one LDS tile ----------------------------------------------------------------------------------------------
def test_many_rows():
    m, n, k = 1100, 700, 8
    V, W0 = blob_data(m, n, k)
    W, H, assigned, ferr, gap = co.kmeans(V, k, W=W0, niter=3)
    assert gap >= 1e-4
    check_kmeans(device_kmeans(V, k, W0, niter=3), W, H, assigned, ferr, "kmeans 1100x700")
    H0 = np.random.RandomState(5).random_sample((k, n))
    Wc, Hc, fc = co.cmeans(V, W0, H0, niter=3)
    mdl = pymf_amd.Cmeans(V, num_bases=k)
    mdl.W, mdl.H = np.array(W0), H0.copy()
    mdl.factorize(niter=3)
    assert rel_fro(mdl.W, Wc, "cmeans 1100x700 W") < TOL
    assert rel_fro(mdl.H, Hc, "cmeans 1100x700 H") < TOL
    close(mdl.ferr, fc, rtol=TOL, what="cmeans 1100x700 ferr")


# ---- 6: centres with one member or none keep their column (kmeans.py:86) -----------------------------------------------------------
def test_small_clusters_keep_their_centre():
    rs = np.random.RandomState(11)
    V = (0.1 * rs.randn(16, 40)).astype(np.float32)
    V[:, :20] += 1.0                                   # two real clusters, around 1 and around 0 ...
    V[:, 7] = 10.0                                     # ... and one outlier
    W0 = np.zeros((16, 4), dtype=np.float32)
    W0[:, 0] = 1.0
    W0[:, 2] = 9.75                                    # gets sample 7 alone
    W0[:, 3] = -50.0                                   # gets nobody
    W0 += (0.01 * rs.randn(16, 4)).astype(np.float32)
    W, H, assigned, ferr, gap = co.kmeans(V, 4, W=W0, niter=3)
    assert np.sum(assigned == 2) == 1 and np.sum(assigned == 3) == 0 and gap >= 1e-4
    mdl = device_kmeans(V, 4, W0.astype(np.float64), niter=3)
    check_kmeans(mdl, W, H, assigned, ferr, "kmeans small clusters")
    assert np.array_equal(mdl.W[:, 2:], W0[:, 2:].astype(np.float64))


# ---- 7: single hooks, partial loops, the hook loop ---------------------------------------------------------------------------------
def test_kmeans_single_hooks():
    m, n, k = BLOB_CASES[2]
    V, W0 = blob_data(m, n, k)
    Vd = V.astype(np.float64)
    mdl = pymf_amd.Kmeans(V, num_bases=k)
    mdl.W, mdl.H = np.array(W0), np.zeros((k, n))
    mdl.update_h()
    assigned, H, gap = co.kmeans_update_h(Vd, W0)
    assert np.array_equal(mdl.assigned, assigned) and np.array_equal(mdl.H, H)
    close(mdl.frobenius_norm(), co.frobenius(Vd, W0, H), rtol=TOL, what="kmeans hook frobenius")
    mdl.update_w()
    W1 = co.kmeans_update_w(Vd, W0, assigned)
    assert rel_fro(mdl.W, W1, "kmeans hook update_w") < TOL
    mdl.assigned = np.roll(assigned, 1)                # a caller's assignment is what update_w uses (kmeans.py:84)
    mdl.update_w()
    assert rel_fro(mdl.W, co.kmeans_update_w(Vd, W1, np.roll(assigned, 1)), "kmeans hook update_w, caller's assigned") < TOL


def test_cmeans_single_hooks():
    m, n, k = BLOB_CASES[2]
    V, W0 = blob_data(m, n, k)
    Vd = V.astype(np.float64)
    H0 = np.random.RandomState(3).random_sample((k, n))
    mdl = pymf_amd.Cmeans(V, num_bases=k)
    mdl.W, mdl.H = np.array(W0), H0.copy()
    mdl.update_w()                                     # the sums of the caller's H: no pass preceded
    W1 = co.cmeans_update_w(Vd, W0, H0)
    assert rel_fro(mdl.W, W1, "cmeans hook update_w") < TOL
    mdl.W = np.array(W0)
    mdl.update_h()
    H1 = co.cmeans_update_h(Vd, W0)
    assert rel_fro(mdl.H, H1, "cmeans hook update_h") < TOL
    close(mdl.frobenius_norm(), co.frobenius(Vd, W0, H1), rtol=TOL, what="cmeans hook frobenius")


@pytest.mark.parametrize("cw,ch", [(False, True), (True, False)])
def test_partial_loops(cw, ch):
    m, n, k = BLOB_CASES[2]
    V, W0 = blob_data(m, n, k)
    W, H, assigned, ferr, gap = co.kmeans(V, k, W=W0, niter=4, compute_w=cw, compute_h=ch)
    check_kmeans(device_kmeans(V, k, W0, niter=4, compute_w=cw, compute_h=ch), W, H, assigned, ferr, "kmeans cw=%s ch=%s" % (cw, ch))
    H0 = np.random.RandomState(9).random_sample((k, n))
    Wc, Hc, fc = co.cmeans(V, W0, H0, niter=4, compute_w=cw, compute_h=ch)
    mdl = pymf_amd.Cmeans(V, num_bases=k)
    mdl.W, mdl.H = np.array(W0), H0.copy()
    mdl.factorize(niter=4, compute_w=cw, compute_h=ch)
    assert len(mdl.ferr) == len(fc)
    assert rel_fro(mdl.W, Wc, "cmeans cw=%s ch=%s W" % (cw, ch)) < TOL
    assert rel_fro(mdl.H, Hc, "cmeans cw=%s ch=%s H" % (cw, ch)) < TOL
    close(mdl.ferr, fc, rtol=TOL, what="cmeans cw=%s ch=%s ferr" % (cw, ch))


def test_overridden_converged_takes_the_hook_loop():
    calls = []

    class Counting(pymf_amd.Kmeans):
        def converged(self, i):
            calls.append(i)
            return pymf_amd.Kmeans.converged(self, i)

    m, n, k = BLOB_CASES[0]
    V, W0 = blob_data(m, n, k)
    W, H, assigned, ferr, gap = kmeans_oracle(m, n, k)
    mdl = device_kmeans(V, k, W0, cls=Counting, niter=6)
    assert calls == [2]
    check_kmeans(mdl, W, H, assigned, ferr, "kmeans hook loop")


# ---- 8: determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Kmeans", "Cmeans"])
def test_two_runs_give_the_same_bits(cls):
    m, n, k = BLOB_CASES[0]
    V, W0 = blob_data(m, n, k)
    runs = []
    for _ in range(2):
        mdl = getattr(pymf_amd, cls)(V, num_bases=k)
        mdl.W = np.array(W0)
        if cls == "Cmeans":
            mdl.H = np.random.RandomState(1).random_sample((k, n))
        mdl.factorize(niter=6)
        runs.append((mdl.W.copy(), mdl.H.copy(), mdl.ferr.copy(), np.array(getattr(mdl, "assigned", 0))))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- 9: unstructured data at large n: properties, not trajectories ---------------------------------------------------------------
def test_kmeans_properties_on_uniform_data():
    m, n, k, niter = 64, 5000, 8, 8
    V = np.random.RandomState(21).random_sample((m, n)).astype(np.float32)
    Vd = V.astype(np.float64)
    random.seed(0)
    full = device_kmeans(V, k, niter=niter)
    ferr = full.ferr.copy()
    assert np.array_equal(full.H.sum(axis=0), np.ones(n)) and set(np.unique(full.H)) <= {0.0, 1.0}
    assert np.array_equal(np.argmax(full.H, axis=0), full.assigned)
    assert np.all(ferr[1:] <= ferr[:-1] * (1 + 1e-6)), ferr
    for it in range(1, len(ferr) + 1):                 # W_i, H_i: the same seed, i iterations
        random.seed(0)
        mdl = device_kmeans(V, k, niter=it)
        if len(mdl.ferr) < it:                         # (converged() cut the history: nmf.py:198-202)
            break
        assert mdl.ferr[it - 1] == ferr[it - 1]
        close(mdl.ferr[it - 1], co.frobenius(Vd, mdl.W, mdl.H), rtol=TOL, what="kmeans uniform ferr[%d]" % (it - 1))
    full.update_w()                                    # the centres of the device's own assignment
    for j in range(k):
        idx = np.where(full.assigned == j)[0]
        if len(idx) > 1:
            assert rel_fro(full.W[:, j], Vd[:, idx].sum(axis=1) / len(idx), "kmeans uniform centre %d" % j) < TOL
