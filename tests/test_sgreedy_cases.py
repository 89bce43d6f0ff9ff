"""The conditions under which the device comparison of tests/test_gpu_sgreedy.py means something, on the oracles alone (no
GPU): in every round of every case the literal float64 oracle, its float32 twin and the reference goldens pick the same column,
the winner leads the runner-up by at least GAP_FACTOR x the worst relative score difference between twin and oracle, and the
twin's deviations of _v, H and ferr are the figures the device tolerances are made of."""
import functools

import numpy as np
import pytest

import sgreedy_cases as gc
import sgreedy_oracle as sg
import sivm_cases as sc
import sivm_oracle as so
from conftest import load_golden

NAMES = sorted(gc.CASES)
SELECT_NAMES = NAMES + sorted(gc.PANEL_CASES)
F1_RTOL = 2.0 ** -24
GOLDENS = ["sgreedy_doc_2x3_k2", "sgreedy_doc_userw", "sgreedy_37x29_k5", "sgreedy_29x300_k6_l2", "sgreedy_29x300_k6_l1",
           "sgreedy_29x300_k6_cosine", "sgreedy_29x300_k6_origin"]


@functools.lru_cache(maxsize=None)
def twin(name):
    c = gc.case(name)
    scores = []
    select, W, v, picks = sg.update_w_twin(c["V"].astype(np.float64), c["k"], c["metric"], c["init"], scores=scores)
    return dict(select=select, W=W, v=v, picks=picks, scores=scores)


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_same_pick_in_every_round_with_a_wide_lead(name):
    c, t = gc.case(name), twin(name)
    assert len(c["scores"]) == len(t["scores"]) == c["k"] - 1
    assert t["picks"] == c["picks"] and t["select"] == c["select"]
    worst = max(float(np.max(np.abs(b - a)) / np.max(a)) for a, b in zip(c["scores"], t["scores"]))
    lead = min(min(gc.lead(a, c["special"]), gc.lead(b, c["special"])) for a, b in zip(c["scores"], t["scores"]))
    print("%s: worst relative score difference twin / oracle %.3e, smallest lead %.3e (%.0f x)" % (name, worst, lead, lead / worst))
    assert lead >= gc.GAP_FACTOR * worst


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_selection_reaches_its_range(name):
    c = gc.case(name)
    n = c["V"].shape[1]
    assert len(set(c["select"])) == c["k"]
    assert c["select"] == sorted(c["picks"][:-1]) + c["picks"][-1:]
    if c["init"] == "fastmap":
        assert sorted(c["select"]) == sorted(c["verts"])
    else:
        assert c["select"][0] == -1 and np.array_equal(c["W"][:, 0], c["V"][:, -1].astype(np.float64))
    if c["special"] in ("ends", "trip2"):   # winners in the first and in the last workgroup
        assert min(c["select"]) < 64 and max(c["select"]) >= n - 64
    if c["special"] == "trip2":             # a winner that only the second trip of the quad loop sees
        assert gc.TRIP2_COLUMN in c["select"]
    if name in gc.PANEL_CASES:
        assert (c["V"].shape[0], n) in {(s[0], s[1]) for s in sc.PANEL_CASES.values()}
    else:
        assert -(-n // 64) <= 1024          # one panel per workgroup


def test_the_tie_is_a_tie_in_a_volume_round():
    c = gc.case("sgreedy_16x640_k4_tie")
    same = [j for j in range(gc.TIE_COLUMN) if np.array_equal(c["V"][:, j], c["V"][:, gc.TIE_COLUMN])]
    assert len(same) == 1
    assert same[0] in c["select"] and gc.TIE_COLUMN not in c["select"]          # the lower index wins
    tied = [bool(np.sort(s)[-1] == np.sort(s)[-2]) for s in c["scores"]]
    assert any(tied)
    r = tied.index(True)
    assert c["picks"][r + 1] == same[0] and int(np.argmax(c["scores"][r])) == same[0]
    assert twin("sgreedy_16x640_k4_tie")["scores"][r][same[0]] == twin("sgreedy_16x640_k4_tie")["scores"][r][gc.TIE_COLUMN]


def test_the_shapes_cover_what_they_say():
    assert {gc.CASES[n][0] % 4 for n in NAMES} == {0, 1, 2, 3}
    assert {29, 30, 31, 32} <= {gc.CASES[n][0] for n in NAMES}
    assert any(gc.CASES[n][0] > 64 for n in NAMES)
    assert any(gc.CASES[n][1] == 300 for n in NAMES)
    assert {gc.CASES[n][4] for n in NAMES} == {"l2", "l1", "cosine"}
    assert any(gc.CASES[n][5] == "origin" for n in NAMES)
    assert any(gc.CASES[n][2] == 64 and gc.CASES[n][0] >= 80 for n in NAMES)


def golden_v(g):
    if "case" in g:
        m, n, k, seed, _, _, special = gc.CASES[str(g["case"])]
        return gc.data(m, n, k, seed, special)[0]
    return g["V"]


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_reproduces_golden(name):
    """select and W exactly, H and ferr to the float64 tolerances of the other golden tests.  _v to one float32 rounding of
    f1: vol.py:30 makes j a float32, and under the NumPy and SciPy that wrote the goldens f1 comes out as a float32 from t = 2
    on (relative error at most 2^-24 on f1, half of that on its root); the oracle keeps f1 in float64."""
    g = load_golden(name)
    V = golden_v(g).astype(np.float64)
    if "select" in g:
        select, W, v, _ = sg.update_w(V, int(g["k"]), str(g["metric"]), str(g["init"]))
        assert select == [int(s) for s in g["select"]]
        assert np.array_equal(W, g["W"])
        assert np.allclose(v, g["v"], rtol=F1_RTOL, atol=0.0)
        for label, t in (("twin", sg.update_w_twin(V, int(g["k"]), str(g["metric"]), str(g["init"]))),):
            assert t[0] == select, label
        if "case" in g:
            c = gc.case(str(g["case"]))
            assert select == c["select"] and np.allclose(c["v"], g["v"], rtol=F1_RTOL, atol=0.0)
    H, ferr = so.update_h(V, g["W"])
    assert np.abs(H - g["H"]).max() <= 1e-10
    assert abs(ferr - g["ferr"][0]) <= 1e-10 * max(1.0, g["ferr"][0])
    if name == "sgreedy_29x300_k6_cosine":
        assert bool(g["cosine_patched"])


@functools.lru_cache(maxsize=None)
def deviation(name):
    """(_v relative, H relative Frobenius, ferr relative): the twin and the float32 H step against the all-float64 oracle"""
    c, t = gc.case(name), twin(name)
    dv = max([abs(a - b) / a for a, b in zip(c["v"], t["v"])] or [0.0])
    H32, ferr32 = so.update_h(c["V"].astype(np.float64), c["W"], True, True, True, True)
    Vr, Wr, S, F = so.products(c["V"].astype(np.float64), c["W"], True, True, True)
    Hs, _ = so.simplex_rounds(S, F)                              # the device's multiplier search, stopping rule included
    ferrs = float(np.sqrt(((Vr - Wr.dot(Hs)) ** 2).sum()))
    dh = max(np.linalg.norm(H - c["H"]) / np.linalg.norm(c["H"]) for H in (H32, Hs))
    return dv, dh, max(abs(f - c["ferr"]) / c["ferr"] for f in (ferr32, ferrs))


@pytest.mark.parametrize("name", NAMES)
def test_twin_deviation(name):
    dv, dh, df = deviation(name)
    print("%s: _v deviation %.3e, H deviation %.3e, ferr deviation %.3e" % (name, dv, dh, df))
    assert dv <= gc.MEASURED_V * 1.001 and dh <= gc.MEASURED_H * 1.001 and df <= gc.MEASURED_FERR * 1.001


def test_the_measured_figures_are_attained():
    dev = [deviation(name) for name in NAMES]
    for i, fig in enumerate((gc.MEASURED_V, gc.MEASURED_H, gc.MEASURED_FERR)):
        assert max(d[i] for d in dev) >= fig * 0.999
    assert (gc.V_TOL, gc.H_TOL, gc.FERR_TOL) == (4.0 * gc.MEASURED_V, 4.0 * gc.MEASURED_H, 4.0 * gc.MEASURED_FERR)
