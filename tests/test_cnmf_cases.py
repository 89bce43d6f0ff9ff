"""The cases of tests/cnmf_cases.py leave room for float32 and reach what they are meant for (no GPU): a failure of
tests/test_gpu_cnmf_cases.py on the device is then the kernel's, not the case's.  (a) The k-means of every planted case
returns the planted labels with a relative distance gap >= 1e-2 (C's error moves a distance by ~3e-7).
(b) The float64 oracle rerun on a C formed in float32 and with W rounded to float32 -- what the float32 data path costs
whatever the arithmetic -- stays within a quarter of the device tolerance on every quantity the device test compares.
(c) The cancellation case crosses 1e-3 tr(C) strictly inside a 32-iteration chunk.  (d) The shapes reach every kernel width
at both ends, np = 64 .. 256 and both kinds of Gram chunks."""
import numpy as np
import pytest

import cnmf_cases as cc

TOL = {"G": 1e-5, "H": 1e-5, "W": 2e-5, "ferr": 1e-5}       # tests/test_gpu_cnmf_cases.py, DESIGN.md section 4
GAP = 1e-2
EPS = 1e-8                                                 # nmf.py:69


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))


# ---- (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.PLANTED_CASES, ids=cc.case_id)
def test_kmeans_returns_the_planted_labels(c):
    _, sel, labels = cc.data(c)
    H0, G0, assigned, gap = cc.start(c)
    counts = np.bincount(assigned, minlength=c.k)
    print(cc.case_id(c), "gap %.3g" % gap, "members %d .. %d" % (counts.min(), counts.max()))
    assert np.array_equal(assigned, labels)
    assert np.array_equal(assigned[sel], np.arange(c.k))
    assert gap >= GAP
    if (c.m, c.n, c.k) in cc.ONE_MEMBER_SHAPES:            # k_kmeans_update must leave these centres where they are
        assert counts.min() == 1
        assert np.sum(counts == 1) == (c.k if c.n == c.k else c.k - (c.n - c.k))


def test_the_shifted_cases_are_mixed_sign():
    for c in cc.PLANTED_CASES:
        neg = float(np.mean(cc.gram32(c) < 0))
        if c.m >= 16:                                      # (three centres in five dimensions may well all point the same way)
            assert (0.4 <= neg <= 0.6) if c.shift else neg == 0.0, (cc.case_id(c), neg)


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def room(tag, ref, f32, compute_err=True):
    W, H, G, ferr = ref
    Ws, Hs, Gs, ferr_s = f32
    assert len(ferr_s) == len(ferr)
    got = {"G": rel(Gs, G), "H": rel(Hs, H), "W": rel(Ws, W)}
    if compute_err:
        got["ferr"] = float(np.max(np.abs(ferr_s - ferr) / ferr))
    else:
        assert not ferr.any() and not ferr_s.any()
    print(tag, {q: "%.2g of %.2g" % (v, TOL[q] / 4) for q, v in got.items()})
    for q, v in got.items():
        assert v <= TOL[q] / 4, (q, v)


@pytest.mark.parametrize("r", cc.ALL_RUNS, ids=cc.run_id)
def test_run_leaves_room_for_float32(r):
    ferr = cc.run_oracle(r)[3]
    room(cc.run_id(r), cc.run_oracle(r), cc.run_oracle(r, f32=True), r.compute_err)
    # no run converges, and none comes near it: float32 noise in an error cannot raise a false stop
    assert len(ferr) == r.niter
    if r.compute_err and r.niter > 2:
        assert np.min(np.abs(np.diff(ferr))[1:]) / r.c.n >= 100 * EPS


def test_replaced_data_leave_room_for_float32():
    room("replaced data", cc.replaced_oracle(), cc.replaced_oracle(f32=True))
    assert len(cc.replaced_oracle()[3]) == cc.REPLACE_NITER
    assert cc.REPLACE_FROM._replace(shift=0.5) == cc.REPLACE_TO and cc.REPLACE_FROM in cc.WIDTH_CASES


def test_the_dense_starts_are_dense():
    for c in cc.ONE_STEP_CASES:
        H0, G0 = cc.dense_start(c)
        assert H0.shape == (c.k, c.n) and G0.shape == (c.n, c.k)
        assert 0.4 < np.median(H0) < 0.6 and 0.4 / 3 < np.median(G0) < 0.6 / 3


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def crossing(r):
    """e^2 / tr(C) per iteration, and the first iteration where it is below 1e-3 (None: never)."""
    q = cc.run_oracle(r)[3] ** 2 / cc.trace(r.c)
    below = np.where(q < 1e-3)[0]
    return q, (int(below[0]) if len(below) else None)


def test_the_loop_runs_enter_the_free_running_loop_and_stay_in_it():
    """cnmf_factorize: iteration 0 by hand, then chunks while e^2 > 1e-2 tr(C) at the start and two iterations are left;
    none of these runs comes near the 1e-3 of the fallback.  The second of two calls of 35 iterations starts below 1e-2 and
    runs by hand throughout; the second of two calls of 8 starts above it and runs in chunks again."""
    for r in cc.LOOP_RUNS + cc.NO_G_RUNS:
        q, at = crossing(r)
        assert q[0] > 2e-2 and at is None and q.min() > 2e-3, (cc.run_id(r), q[0], q.min())
    q, at = crossing(cc.TWICE_RUN)
    assert at is None and q.min() > 2e-3 and q.max() < 0.9e-2
    q, at = crossing(cc.TWICE_EARLY_RUN)
    assert at is None and q[0] > 1.1e-2
    assert cc.LOOP_NITER == (1, 2, 3, 1 + cc.CHUNK, 2 + cc.CHUNK, 70)      # no chunk, no chunk, a chunk of 2, 32 + 0, 32 + 1, 32 + 32 + 5


def test_the_cancellation_case_crosses_inside_a_chunk():
    q, at = crossing(cc.CANCEL_RUN)
    ferr = cc.run_oracle(cc.CANCEL_RUN)[3]
    print("e^2 / tr(C): first %.4g, %.5g at %d, %.5g at %d" % (q[0], q[at - 1], at - 1, q[at], at))
    assert q[0] > 1e-2                                     # the free-running loop starts after iteration 0
    assert at == 55 and (at - 1) % cc.CHUNK not in (0, cc.CHUNK - 1)      # chunks: 1 .. 32, 33 .. 64, 65 .. 69
    assert np.all(q[:at] >= 1.01e-3) and np.all(q[at:] <= 0.99e-3)        # 1 % of margin on either side of the crossing
    assert len(ferr) == cc.CANCEL_NITER                    # no convergence: iterations 55 .. 69 run by hand
    assert np.min(np.abs(np.diff(ferr))[1:]) / cc.CANCEL_CASE.n >= 100 * EPS


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def test_the_width_cases_reach_the_ranges_they_are_meant_for():
    """pmf_create: NT = 1, 2, 4, 8 for k <= 16, 32, 64, 128, KP = 16 NT, np = n rounded up to 64.  ensure_vgram (dense):
    gchunks = min(512, mp / 16), rpc = 16 ceil((mp / 16) / gchunks), then gchunks = ceil(mp / rpc)."""
    g = [cc.geometry(*s) for s in cc.WIDTH_SHAPES]
    # NT, KP, np, k-step rounds of k_cnmf_split_gemm, zero rows k .. KP, zero columns n .. np, rpc, Gram chunks
    seen = [(d["NT"], d["KP"], d["np"], d["rounds"], d["pad_rows"], d["pad_cols"], d["rpc"], d["gchunks"]) for d in g]
    assert seen == [(1, 16, 64, 1, 0, 0, 16, 8), (2, 32, 128, 2, 15, 63, 16, 8), (2, 32, 192, 3, 0, 62, 16, 4),
                    (4, 64, 256, 4, 31, 56, 16, 8), (4, 64, 192, 3, 0, 0, 16, 12), (8, 128, 192, 3, 63, 62, 16, 8),
                    (8, 128, 256, 4, 28, 56, 16, 8), (8, 128, 128, 2, 0, 0, 16, 20), (4, 64, 128, 2, 17, 58, 16, 8),
                    (1, 16, 64, 1, 13, 0, 16, 4), (2, 32, 64, 1, 15, 47, 16, 8), (1, 16, 64, 1, 10, 0, 32, 258)]
    ks = {}
    for (m, n, k), d in zip(cc.WIDTH_SHAPES, g):
        ks.setdefault(d["NT"], set()).add(k)
    assert {nt: (min(v), max(v)) for nt, v in ks.items()} == {1: (3, 16), 2: (17, 32), 4: (33, 64), 8: (65, 128)}
    assert {d["np"] for d in g} == {64, 128, 192, 256}
    assert {d["rpc"] for d in g} == {16, 32}
    assert any(n == k for (m, n, k) in cc.WIDTH_SHAPES) and any(m < 16 for (m, n, k) in cc.WIDTH_SHAPES)
    # every width has a one-step case and a mixed-sign width case
    assert {cc.geometry(c.m, c.n, c.k)["NT"] for c in cc.ONE_STEP_CASES} == {1, 2, 4, 8}
    assert {cc.geometry(c.m, c.n, c.k)["NT"] for c in cc.WIDTH_CASES if c.shift} == {1, 2, 4, 8}
