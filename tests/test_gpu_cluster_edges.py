"""pymf_amd.Kmeans / pymf_amd.Cmeans on the MI355X where tests/test_gpu_cluster.py does not reach: more than one 64-column
panel per workgroup (n > 65 536: the loop over a workgroup's panels, a one-tile W staged once, phase B over several panels,
the clipped last workgroup, sums over several hundred slabs), data away from the origin and tight clusters (the expanded
distance ||w||^2 - 2 w.v + ||v||^2 cancels there; the kernel takes both relative to the row means of the data), and the
state that follows the data.  The cases and their float64 oracle results: tests/cluster_edge_cases.py; that they leave room
for float32: tests/test_cluster_edge_cases.py.  Tolerance: DESIGN.md section 4, 2e-5."""
import numpy as np
import pytest

import cluster_edge_cases as ec
import cluster_oracle as co
import pymf_amd
from conftest import close, rel_fro
from test_gpu_cluster import TOL, check_kmeans, device_kmeans

pytestmark = pytest.mark.gpu

assert TOL == 2e-5
WIDE = ec.PANEL_CASES[0]                                   # 8 x 65 570: two panels per workgroup


def cmeans_model(c, W, H):
    mdl = pymf_amd.Cmeans(ec.data(c)[0], num_bases=c.k)
    mdl.W, mdl.H = np.array(W), np.array(H)
    return mdl


def check_cmeans(mdl, W, H, ferr, tag):
    assert len(mdl.ferr) == len(ferr)
    assert rel_fro(mdl.W, W, tag + " W") < TOL
    assert rel_fro(mdl.H, H, tag + " H") < TOL
    close(mdl.ferr, ferr, rtol=TOL, what=tag + " ferr")


# ---- 1: panel ranges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.PANEL_CASES, ids=ec.case_id)
def test_kmeans_panel_ranges(c):
    V, W0 = ec.data(c)
    W, H, assigned, ferr, gap = ec.kmeans_oracle(c)
    assert gap >= 1e-4
    check_kmeans(device_kmeans(V, c.k, W0, niter=ec.NITER), W, H, assigned, ferr, "kmeans " + ec.case_id(c))


@pytest.mark.parametrize("c", ec.PANEL_CASES, ids=ec.case_id)
def test_cmeans_panel_ranges(c):
    """From the memberships of the perturbed true centres (update_h(), then the loop): H is far from uniform."""
    W, H, ferr = ec.cmeans_oracle(c, from_centres=True)
    mdl = cmeans_model(c, ec.data(c)[1], np.zeros((c.k, c.n)))
    mdl.update_h()
    mdl.factorize(niter=ec.NITER)
    check_cmeans(mdl, W, H, ferr, "cmeans " + ec.case_id(c))


def test_sums_only_pass_over_panel_ranges():
    """update_w() that no pass preceded (assign = 0): Cmeans on a caller's H, Kmeans on a caller's assignment."""
    c = WIDE
    V, W0 = ec.data(c)
    Vd = V.astype(np.float64)
    H0 = ec.random_h0(c)
    mdl = cmeans_model(c, W0, H0)
    mdl.update_w()
    assert rel_fro(mdl.W, co.cmeans_update_w(Vd, W0, H0), "cmeans sums only, caller's H") < TOL
    mdl = pymf_amd.Kmeans(V, num_bases=c.k)
    mdl.W, mdl.H = np.array(W0), np.zeros((c.k, c.n))
    mdl.update_h()
    assigned = co.kmeans_update_h(Vd, W0)[0]
    assert np.array_equal(mdl.assigned, assigned)
    mdl.assigned = np.roll(assigned, 1)
    mdl.update_w()
    assert rel_fro(mdl.W, co.kmeans_update_w(Vd, W0, np.roll(assigned, 1)), "kmeans sums only, caller's assigned") < TOL


@pytest.mark.parametrize("cls", ["Kmeans", "Cmeans"])
def test_two_runs_over_panel_ranges_give_the_same_bits(cls):
    c = WIDE
    V, W0 = ec.data(c)
    runs = []
    for _ in range(2):
        mdl = getattr(pymf_amd, cls)(V, num_bases=c.k)
        mdl.W = np.array(W0)
        if cls == "Cmeans":
            mdl.H = ec.random_h0(c)
        mdl.factorize(niter=ec.NITER)
        runs.append((mdl.W.copy(), mdl.H.copy(), mdl.ferr.copy(), np.array(getattr(mdl, "assigned", 0))))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- 2: cancellation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.CANCEL_CASES, ids=ec.case_id)
def test_kmeans_cancellation(c):
    V, W0 = ec.data(c)
    W, H, assigned, ferr, gap = ec.kmeans_oracle(c)
    assert gap >= 1e-4
    tag = "kmeans " + ec.case_id(c)
    mdl = device_kmeans(V, c.k, W0, niter=ec.NITER)
    print(tag, "W %.3g ferr %.3g" % (np.linalg.norm(mdl.W - W) / np.linalg.norm(W),
                                     np.max(np.abs(mdl.ferr - ferr) / ferr) if len(mdl.ferr) == len(ferr) else np.nan))
    check_kmeans(mdl, W, H, assigned, ferr, tag)
    if c.offset <= ec.CENTRED_MAX_OFFSET:                  # (||W|| ~ offset sqrt(m k) would hide an error of the centres)
        mu = ec.row_mean(c)
        assert rel_fro(mdl.W - mu, W - mu, tag + " W - mu") < TOL


@pytest.mark.parametrize("c", ec.CANCEL_CASES, ids=ec.case_id)
def test_cmeans_update_h_cancellation(c):
    """The memberships of the perturbed true centres: every distance counts, none of them is near 1 / k."""
    mdl = cmeans_model(c, ec.data(c)[1], np.zeros((c.k, c.n)))
    mdl.update_h()
    assert rel_fro(mdl.H, ec.cmeans_hook_oracle(c), "cmeans hook H " + ec.case_id(c)) < TOL


@pytest.mark.parametrize("c", ec.CANCEL_CASES, ids=ec.case_id)
def test_cmeans_cancellation(c):
    W, H, ferr = ec.cmeans_oracle(c)
    mdl = cmeans_model(c, ec.data(c)[1], ec.random_h0(c))
    mdl.factorize(niter=ec.NITER)
    check_cmeans(mdl, W, H, ferr, "cmeans " + ec.case_id(c))


# ---- 3: state that follows the data -------------------------------------------------------------------------------------------
A, B = ec.CANCEL_CASES[0], ec.CANCEL_CASES[1]              # the same clusters at offset 10 and at offset 100


def test_kmeans_follows_replaced_data():
    (VA, W0), (VB, W0B) = ec.data(A), ec.data(B)
    VBd = VB.astype(np.float64)
    mdl = pymf_amd.Kmeans(VA, num_bases=A.k)
    mdl.W, mdl.H = np.array(W0), np.zeros((A.k, A.n))
    mdl.update_h()
    assigned = co.kmeans_update_h(VA.astype(np.float64), W0)[0]
    assert np.array_equal(mdl.assigned, assigned)
    mdl.data = VB
    mdl.update_w()                                         # the old assignment, the sums of the new data
    assert rel_fro(mdl.W, co.kmeans_update_w(VBd, W0, assigned), "kmeans update_w on replaced data") < TOL
    W1 = mdl.W.copy()
    mdl.update_h()                                         # the row means of the new data
    assigned, H, gap = co.kmeans_update_h(VBd, W1)
    assert gap >= 1e-4
    assert np.array_equal(mdl.assigned, assigned) and np.array_equal(mdl.H, H)
    close(mdl.frobenius_norm(), co.frobenius(VBd, W1, H), rtol=TOL, what="kmeans frobenius on replaced data")
    mdl.W = np.array(W0B)                                  # the loop and its ferr on the new data
    W, H, assigned, ferr, gap = ec.kmeans_oracle(B)
    mdl.factorize(niter=ec.NITER)
    check_kmeans(mdl, W, H, assigned, ferr, "kmeans loop on replaced data")


def test_cmeans_follows_replaced_data():
    (VA, W0), (VB, W0B) = ec.data(A), ec.data(B)
    VBd = VB.astype(np.float64)
    mdl = cmeans_model(A, W0, np.zeros((A.k, A.n)))
    mdl.update_h()
    H1 = mdl.H.copy()
    assert rel_fro(H1, ec.cmeans_hook_oracle(A), "cmeans hook H before the replacement") < TOL
    mdl.data = VB
    mdl.update_w()                                         # the old H, the sums of the new data
    assert rel_fro(mdl.W, co.cmeans_update_w(VBd, W0, H1), "cmeans update_w on replaced data") < TOL
    W1 = mdl.W.copy()
    mdl.update_h()                                         # the row means of the new data
    assert rel_fro(mdl.H, co.cmeans_update_h(VBd, W1), "cmeans update_h on replaced data") < TOL
    mdl.W = np.array(W0B)
    mdl.update_h()
    assert rel_fro(mdl.H, ec.cmeans_hook_oracle(B), "cmeans hook H after the replacement") < TOL


def test_kmeans_update_w_keeps_the_columns_of_a_replaced_w():
    """update_h(), W = W2, update_w(): centres with fewer than two members keep W2's columns, the others the member means."""
    V, W0 = ec.small_clusters()
    Vd = V.astype(np.float64)
    mdl = pymf_amd.Kmeans(V, num_bases=4)
    mdl.W, mdl.H = W0.astype(np.float64), np.zeros((4, 40))
    mdl.update_h()
    assigned = co.kmeans_update_h(Vd, W0.astype(np.float64))[0]
    assert np.array_equal(mdl.assigned, assigned)
    assert np.sum(assigned == 2) == 1 and np.sum(assigned == 3) == 0
    W2 = (1.5 * W0 + 0.25).astype(np.float32).astype(np.float64)
    mdl.W = W2.copy()
    mdl.update_w()
    assert np.array_equal(mdl.W[:, 2:], W2[:, 2:])
    for j in range(2):
        assert rel_fro(mdl.W[:, j], Vd[:, assigned == j].mean(axis=1), "kmeans member mean %d under a replaced W" % j) < TOL
