"""The cases of tests/cluster_edge_cases.py leave room for float32 (no GPU): a failure of tests/test_gpu_cluster_edges.py on
the device is then the kernel's, not the case's.  (1) No Kmeans run comes within 1e-4 of ||v|| of a tie between two centres
(an fp32 dot product of m terms is off by at most m 2^-24 of ||w|| ||v||).  (2) The float64 oracle with W and
H rounded to float32 after every step -- what float32 STORAGE alone costs, whatever the arithmetic -- stays within a quarter
of the tolerance on every quantity the device test compares."""
import numpy as np
import pytest

import cluster_edge_cases as ec

TOL = 2e-5                                                 # tests/test_gpu_cluster_edges.py, DESIGN.md section 4
ROOM = TOL / 4
GAP = 1e-4
ALL_CASES = ec.PANEL_CASES + ec.CANCEL_CASES


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))


def rel_max(a, b):
    assert len(a) == len(b)
    return float(np.max(np.abs(np.asarray(a) - b) / np.abs(b)))


def test_the_panel_cases_reach_the_ranges_they_are_meant_for():
    """cluster_alloc (pmf_host_cluster.h): at most 1 024 workgroups, panels_per_wg = ceil(panels / 1 024)."""
    seen = []
    for c in ec.PANEL_CASES:
        panels = -(-c.n // 64)
        ppw = -(-panels // min(panels, 1024))
        wgs = -(-panels // ppw)
        seen.append((panels, ppw, wgs, panels - (wgs - 1) * ppw, c.n - (panels - 1) * 64, -(-c.m // 64), -(-c.k // 16)))
    # panels, per workgroup, workgroups, panels of the last workgroup, columns of the last panel, W tiles, 16-base tiles
    assert seen == [(1025, 2, 513, 1, 34, 1, 1), (1025, 2, 513, 1, 34, 2, 1), (2050, 3, 684, 1, 54, 1, 2)]


@pytest.mark.parametrize("c", ALL_CASES, ids=ec.case_id)
def test_kmeans_case_leaves_room_for_float32(c):
    W, H, assigned, ferr, gap = ec.kmeans_oracle(c)
    Ws, Hs, assigned_s, ferr_s, gap_s = ec.kmeans_oracle(c, stored=True)
    mu = ec.row_mean(c)
    got = {"W": rel(Ws, W), "ferr": rel_max(ferr_s, ferr)}
    if c.offset <= ec.CENTRED_MAX_OFFSET:
        got["W - mu"] = rel(Ws - mu, W - mu)
    print(ec.case_id(c), "gap %.3g / stored %.3g" % (gap, gap_s), {q: "%.2g" % v for q, v in got.items()})
    assert gap >= GAP and gap_s >= GAP
    assert len(np.unique(assigned)) == c.k                 # every centre keeps members: none of them is left as it was
    assert np.array_equal(assigned_s, assigned) and np.array_equal(Hs, H)
    for q, v in got.items():
        assert v <= ROOM, (q, v)


@pytest.mark.parametrize("c", ec.CANCEL_CASES, ids=ec.case_id)
def test_cmeans_case_leaves_room_for_float32(c):
    """The update_h() hook from the perturbed true centres, and three iterations from a random H0."""
    W, H, ferr = ec.cmeans_oracle(c)
    Ws, Hs, ferr_s = ec.cmeans_oracle(c, stored=True)
    got = {"hook H": rel(ec.cmeans_hook_oracle(c, stored=True), ec.cmeans_hook_oracle(c)),
           "W": rel(Ws, W), "H": rel(Hs, H), "ferr": rel_max(ferr_s, ferr)}
    print(ec.case_id(c), {q: "%.2g" % v for q, v in got.items()})
    for q, v in got.items():
        assert v <= ROOM, (q, v)


@pytest.mark.parametrize("c", ec.PANEL_CASES, ids=ec.case_id)
def test_cmeans_panel_case_leaves_room_for_float32(c):
    """update_h() from the perturbed true centres, then three iterations."""
    W, H, ferr = ec.cmeans_oracle(c, from_centres=True)
    Ws, Hs, ferr_s = ec.cmeans_oracle(c, stored=True, from_centres=True)
    got = {"W": rel(Ws, W), "H": rel(Hs, H), "ferr": rel_max(ferr_s, ferr)}
    print(ec.case_id(c), {q: "%.2g" % v for q, v in got.items()})
    for q, v in got.items():
        assert v <= ROOM, (q, v)


def test_the_hook_memberships_are_not_uniform():
    """Why the update_h() hook from the true centres is the strong check of the distances: its H is far from 1 / k."""
    for c in ec.CANCEL_CASES:
        H = ec.cmeans_hook_oracle(c)
        assert np.median(H.max(axis=0)) > 0.5, (ec.case_id(c), np.median(H.max(axis=0)))
