"""The conditions under which the device comparison of tests/test_gpu_sivm.py means something, on the float64 oracle alone
(no GPU): a clear argmax at every selection step, the same selections with float32-rounded distances, a well-conditioned
W^T W, a multiplier search that ends well inside the device's cap, and the float32 deviations the tolerances are made of."""
import functools
import os
import re

import numpy as np
import pytest

import sivm_cases as sc
import sivm_oracle as so

NAMES = sorted(sc.CASES)
SELECT_NAMES = NAMES + sorted(sc.PANEL_CASES)       # the panel cases compare selection and W only (sivm_cases.py)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pymf_amd", "csrc")


@functools.lru_cache(maxsize=None)
def f32_products(name):
    c = sc.case(name)
    return so.products(c["V"].astype(np.float64), c["W"], True, True, True)


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_argmax_gap(name):
    c = sc.case(name)
    for step, s in enumerate(c["scores"]):
        o = np.sort(s)[::-1]
        runner_up = o[2] if (c["special"] == "tie" and o[0] == o[1]) else o[1]      # the planted tie: gap to the third
        gap = (o[0] - runner_up) / (o[0] - np.median(s))
        assert gap >= sc.MIN_GAP, "%s step %d: gap %.2e" % (name, step, gap)


def test_the_tie_is_a_tie():
    c = sc.case("16x640_k4_tie")
    assert np.array_equal(c["V"][:, 70], c["V"][:, 600])
    assert 70 in c["select"] and 600 not in c["select"]
    assert any(np.sort(s)[-1] == np.sort(s)[-2] for s in c["scores"])


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_selection_is_stable_under_fp32_and_planted(name):
    c = sc.case(name)
    sel32, _ = so.update_w(c["V"].astype(np.float64), c["k"], c["metric"], c["init"], f32_dist=True)
    assert sel32 == c["select"]
    if c["init"] == "fastmap":
        assert sorted(c["select"]) == sorted(c["verts"])
    if c["special"] in ("ends", "trip2"):   # winners in the first and in the last workgroup; pad columns present
        assert min(c["select"]) < 64 and max(c["select"]) >= c["V"].shape[1] - 64
        assert c["V"].shape[1] % 64 != 0 or c["V"].shape[1] == 65600     # (8 x 65 600: whole panels, see sivm_cases.PANEL_CASES)


def test_the_panel_cases_reach_the_ranges_they_are_meant_for():
    """panel_partition / sivm_select_panels (pmf_host_sivm.h) and the quad loop of k_sivm_pass restated on the shapes, with
    PMF_CL_MAX_WGS read from its header."""
    with open(os.path.join(CSRC, "pmf_cluster.h")) as f:
        max_wgs = int(re.search(r"constexpr int PMF_CL_MAX_WGS = (\d+);", f.read()).group(1))

    def ranges(n):
        panels = -(-n // 64)
        ppw = -(-panels // min(panels, max_wgs))
        wgs = -(-panels // ppw)
        # panels, per workgroup, workgroups, panels of the last workgroup, columns of the last panel, trips of the quad loop
        return panels, ppw, wgs, panels - (wgs - 1) * ppw, n - (panels - 1) * 64, -(-ppw * 16 // 256)

    seen = {name: ranges(c[1]) for name, c in sc.PANEL_CASES.items()}
    assert {seen[n] for n in seen if n.startswith("8x65600")} == {(1025, 2, 513, 1, 64, 1)}
    assert seen["8x1048592_k3_l2"] == (16385, 17, 964, 14, 16, 2)
    assert sc.TRIP2_COLUMN in sc.case("8x1048592_k3_l2")["select"] and sc.TRIP2_COLUMN % (17 * 64) // 4 >= 256   # a winner of the second trip
    assert {c[6] for n, c in sc.PANEL_CASES.items() if n.startswith("8x65600")} == {"l2", "l1", "cosine"}
    assert all(ranges(c[1])[1] == 1 for c in sc.CASES.values())              # none of the full cases gets there


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_condition_number(name):
    W = sc.case(name)["W"]
    assert np.linalg.cond(W.T.dot(W)) <= sc.MAX_COND


@pytest.mark.parametrize("name", NAMES)
def test_rounds_and_fp32_deviation(name):
    c = sc.case(name)
    _, _, S, F = f32_products(name)
    Hr, rounds = so.simplex_rounds(S, F)
    assert rounds.max() <= sc.ROUND_CAP // 2, "%s: %d rounds" % (name, rounds.max())
    assert np.abs(Hr.sum(axis=0) - 1.0).max() <= 1e-6 + 1e-7
    H32, ferr32 = so.update_h(c["V"].astype(np.float64), c["W"], True, True, True, True)
    dh = np.linalg.norm(H32 - c["H"]) / np.linalg.norm(c["H"])
    df = abs(ferr32 - c["ferr"]) / c["ferr"]
    print("%s: H deviation %.3e, ferr deviation %.3e, rounds max %d mean %.2f" % (name, dh, df, rounds.max(), rounds.mean()))
    assert dh <= sc.MEASURED_H * 1.001 and df <= sc.MEASURED_FERR * 1.001   # the figures H_TOL / FERR_TOL are made of
