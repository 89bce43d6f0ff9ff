"""pymf_amd.SIVM on scipy.sparse data, and LAESA's rule on CSC data through the C ABI (the class pymf_amd.LAESA keeps refusing
sparse data: AbiLaesa below does what the class would), on the MI355X, against the float64 oracle on toarray() on the cases of
tests/sivm_sparse_cases.py (where the reference's own run on toarray() is committed as a golden, tests/test_sivm_sparse_cases.py
holds the oracle to it).  select and W must be exact; H within 4 x the oracle's own float32 deviation."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import pymf_amd
import sivm_sparse_cases as ssc
from conftest import rel_fro
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

METRIC_NO = {"l2": 0, "l1": 1, "cosine": 2}


class AbiLaesa(object):
    """LAESA's rule on a SIVM context (sivm_rule = 1) with the surface of the classes that these tests use: dense data through
    pmf_set_v_dense_f32, scipy.sparse data as canonical CSC through pmf_set_v_csc_f32."""

    def __init__(self, data, num_bases=4, dist_measure="l2", init="fastmap"):
        self.data, self.k, self.metric, self.init, self._ctx = data, num_bases, dist_measure, init, None

    def _context(self):
        if self._ctx is None:
            m, n = self.data.shape
            self._ctx = _lib.Context(_lib.ALGO_SIVM, m, n, self.k)
            self._ctx.set_option("sivm_metric", METRIC_NO[self.metric])
            self._ctx.set_option("sivm_init", 1 if self.init == "origin" else 0)
            self._ctx.set_option("sivm_rule", 1)
            if sp.issparse(self.data):
                csc = self.data.tocsc().copy()
                csc.sum_duplicates()
                self._ctx.set_v_csc(csc.indptr, csc.indices, csc.data)
            else:
                self._ctx.set_v_dense(np.asarray(self.data, dtype=np.float32))
        return self._ctx

    def update_w(self):
        ctx = self._context()
        ctx.update_w()
        self.select = [int(s) for s in ctx.get_select()]
        self.W = ctx.get_w()

    def update_h(self):
        ctx = self._context()
        ctx.update_h()
        self.H = ctx.get_h64()

    def factorize(self, compute_h=True, compute_err=False):
        assert not compute_err
        self.update_w()
        if compute_h:
            self.update_h()

    def __del__(self):
        if self._ctx is not None:
            self._ctx.close()


CLASSES = {"sivm": pymf_amd.SIVM, "laesa": AbiLaesa}
_achieved = {}


def ident(p):
    return "-".join(p)


def model(c, rule, metric, init, data=None, team=0):
    mdl = CLASSES[rule](c["csc"] if data is None else data, num_bases=c["k"], dist_measure=metric, init=init)
    if team:
        mdl._context().set_option("sivm_csc_team", team)
    return mdl


def dense_w(c):
    return c["V"][:, c["select"]]


@pytest.fixture(scope="module", autouse=True)
def achieved_errors():
    yield
    if _achieved and os.environ.get("PMF_WRITE_PARITY"):       # (the path to write; the committed copy is profiles/parity_sivm_sparse.json)
        with open(os.environ["PMF_WRITE_PARITY"], "w") as f:
            json.dump(dict(tolerance_H=ssc.H_TOL, achieved_H=_achieved), f, indent=1, sort_keys=True)


@pytest.mark.parametrize("p", ssc.combos(ssc.CASES), ids=ident)
def test_selection_w_and_h(p):
    name, rule, metric, init = p
    c = ssc.case(name, rule, metric, init)
    with_h = ssc.has_h(name, rule, metric, init)
    mdl = model(c, rule, metric, init)
    mdl.factorize(compute_h=with_h, compute_err=False)
    print("%s select %s" % (ident(p), mdl.select))
    assert mdl.select == c["select"]
    assert all(type(s) is int for s in mdl.select)
    W = np.asarray(mdl.W)
    assert type(W) is np.ndarray and W.dtype == np.float32 and np.array_equal(W, dense_w(c))
    if c["special"] == "tie":
        assert 70 in mdl.select and 600 not in mdl.select
    if not with_h:
        return
    Href = ssc.h_oracle(name, rule, metric, init)[0]
    H = np.asarray(mdl.H)
    assert H.dtype == np.float64 and H.shape == Href.shape
    dh = float(rel_fro(H, Href, ident(p) + " H"))
    _achieved[ident(p)] = dh
    print("%s H deviation %.3e (tol %.3e) min H %.3e max |sum - 1| %.3e" % (ident(p), dh, ssc.H_TOL, H.min(), np.abs(H.sum(axis=0) - 1.0).max()))
    assert dh <= ssc.H_TOL
    assert H.min() >= 0.0 and np.abs(H.sum(axis=0) - 1.0).max() <= 1e-5


@pytest.mark.parametrize("p", ssc.combos(ssc.PANEL_CASES), ids=ident)
def test_panel_ranges_select(p):
    """Several 64-column panels per workgroup; vertices in the first and in the last workgroup, and at sivm_cases.TRIP2_COLUMN."""
    name, rule, metric, init = p
    c = ssc.case(name, rule, metric, init)
    mdl = model(c, rule, metric, init)
    mdl.update_w()
    print("%s select %s" % (ident(p), mdl.select))
    assert mdl.select == c["select"]


def team_profile(team, long):
    """256 rows (29 would not hold 3 TEAM + 1 entries), 333 columns: a crowd of columns with 3 TEAM + 1 entries each (long) or
    with 0 .. TEAM - 1 entries, lengths 0 and 1 among them (short) -- small values (|column|_1 <= 7 whatever its length), from
    two entries on one of them on the last row, the crowd's common direction under 'cosine' -- and four vertices on rows of
    their own, each at an angle of its own to that direction."""
    rng = np.random.RandomState(100 + team + long)
    m, n, k = 256, 333, 4
    V = np.zeros((m, n), dtype=np.float32)
    for c in range(n):
        cnt = 3 * team + 1 if long else c % team
        rows = rng.choice(m - 1, size=min(cnt, m - 1), replace=False)
        V[rows, c] = (rng.uniform(0.5, 1.0, size=len(rows)) * 4.0 / max(cnt, 1)).astype(np.float32)
        if cnt >= 2:
            V[rows[0], c] = 0.0
            V[m - 1, c] = 3.0
    for j, c in enumerate(TEAM_VERTICES):
        V[:, c] *= 0.25
        V[j, c] = 20.0 + 5.0 * j
        V[m - 1, c] = 3.0 * (j + 1)
    return sp.csc_matrix(V), k


TEAM_VERTICES = (40, 111, 222, 300)


@pytest.mark.parametrize("long", [0, 1], ids=["short", "long"])
@pytest.mark.parametrize("team", [4, 16, 64])
@pytest.mark.parametrize("rule", sorted(CLASSES))
def test_every_team_forced(rule, team, long):
    """Every TEAM on columns shorter than it and on columns of 3 TEAM + 1 entries, all three metrics.  That the option took effect
    is read from pmf_path_name, which names the team of the next W step: the forced one, and without the option the one that
    the thresholds give for the profile's mean column length."""
    csc, k = team_profile(team, long)
    V64 = csc.toarray().astype(np.float64)
    lens = np.delete(np.diff(csc.indptr), TEAM_VERTICES)
    if long:
        assert lens.min() == lens.max() == 3 * team + 1
    else:
        assert lens.min() == 0 and (lens == 1).any() and lens.max() == team - 1
    mean = csc.nnz / float(csc.shape[1])
    auto = 4 if mean <= 8.0 else 16 if mean <= 48.0 else 64    # PMF_CSC_TEAM4_MAX_MEAN, PMF_CSC_TEAM16_MAX_MEAN
    for metric in ssc.METRICS:
        scores = []
        want = ssc._oracle(V64, k, rule, metric, "fastmap", scores)[0]
        assert ssc.gap(scores, metric) >= ssc.sc.MIN_GAP, (metric, ssc.gap(scores, metric))
        got = {}
        for t in (team, 0):
            mdl = CLASSES[rule](csc, num_bases=k, dist_measure=metric)
            mdl._context().set_option("sivm_csc_team", t)
            mdl.update_w()
            assert mdl._context().path_name == "sivm_csc_teams<%d>" % (t or auto)
            got[t] = mdl.select
            assert np.array_equal(mdl.W, V64[:, want].astype(np.float32))
        print(rule, team, long, metric, got)
        assert got[team] == want and got[0] == want


def test_the_thresholds_choose_every_team():
    """without the option: 16 lanes at 13 entries per column, 64 at 49 and at 193, 4 on the short profile (1.5 on average)"""
    seen = set()
    for team in (4, 16, 64):
        csc, k = team_profile(team, 1)
        mdl = pymf_amd.SIVM(csc, num_bases=k)
        mdl.update_w()
        seen.add(mdl._ctx.path_name)
    assert seen == {"sivm_csc_teams<16>", "sivm_csc_teams<64>"}
    csc, k = team_profile(4, 0)
    mdl = pymf_amd.SIVM(csc, num_bases=k)
    mdl.update_w()
    assert mdl._ctx.path_name == "sivm_csc_teams<4>"


def test_factorize_matches_the_hooks_and_two_runs_give_the_same_bits():
    c = ssc.case("29x300_k6")
    a = model(c, "sivm", "l2", "fastmap")
    a.factorize(compute_err=False)
    b = model(c, "sivm", "l2", "fastmap")
    b.update_w()
    b.update_h()
    assert a.select == b.select == c["select"]
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H)
    W, H = np.array(a.W), np.array(a.H)
    a.factorize(compute_err=False)
    assert a.select == c["select"] and np.array_equal(a.W, W) and np.array_equal(a.H, H)
    assert a.frobenius_norm() == -123456
    assert a._ctx.path_name == "sivm_csc_teams<16>"             # (15.3 stored entries per column)


@pytest.mark.parametrize("rule", sorted(CLASSES))
def test_two_runs_same_bits_of_the_state(rule):
    """the C ABI alone, twice on fresh contexts: selection, W and H bit for bit"""
    c = ssc.case("64x4113_k8", rule)
    out = []
    for _ in range(2):
        ctx = _lib.Context(_lib.ALGO_SIVM, c["csc"].shape[0], c["csc"].shape[1], c["k"])
        try:
            ctx.set_option("sivm_rule", 1 if rule == "laesa" else 0)
            ctx.set_v_csc(c["csc"].indptr, c["csc"].indices, c["csc"].data)
            ctx.update_w()
            ctx.update_h()
            out.append((ctx.get_select().tolist(), ctx.get_w(), ctx.get_h64()))
        finally:
            ctx.close()
    assert out[0][0] == out[1][0] == c["select"]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("fmt", ["csr", "coo"])
def test_sparse_against_dense_and_other_formats(fmt):
    for rule, metric, init in (("sivm", "l2", "fastmap"), ("laesa", "l1", "origin"), ("sivm", "cosine", "fastmap")):
        c = ssc.case("31x300_k6", rule, metric, init)
        dense = CLASSES[rule](c["V"], num_bases=c["k"], dist_measure=metric, init=init)
        dense.update_w()
        other = model(c, rule, metric, init, data=c["csc"].asformat(fmt))
        other.update_w()
        assert dense.select == other.select == c["select"]
        assert np.array_equal(dense.W, other.W)


def test_replacing_data_both_ways_and_in_place_edits():
    a, b = ssc.case("29x300_k6"), ssc.case("29x300_k6_empty")
    ctx = _lib.Context(_lib.ALGO_SIVM, 29, 300, 6)
    try:
        ctx.set_v_csc(a["csc"].indptr, a["csc"].indices, a["csc"].data)
        ctx.update_w()
        assert ctx.get_select().tolist() == a["select"]
        ctx.set_v_dense(b["V"])                            # dense after CSC
        assert ctx.path_name == "sivm_panels"
        ctx.update_w()
        assert ctx.get_select().tolist() == b["select"]
        assert np.array_equal(ctx.get_w(), b["V"][:, b["select"]])
        ctx.update_h()
        ctx.frobenius()                                    # (dense data: the norm exists again)
        ctx.set_v_csc(a["csc"].indptr, a["csc"].indices, a["csc"].data)   # CSC after dense
        ctx.update_w()
        ctx.update_h()
        assert ctx.get_select().tolist() == a["select"]
        assert np.array_equal(ctx.get_w(), dense_w(a))
        with pytest.raises(_lib.PmfError, match="CSC"):
            ctx.frobenius()
        with pytest.raises(_lib.PmfError, match="dense resident data only"):
            ctx.sivm_select(3, False, 0, 0)
        ctx.set_option("sivm_rule", 2)
        with pytest.raises(_lib.PmfError, match="GMAP: dense data only"):
            ctx.update_w()
    finally:
        ctx.close()
    data = a["csc"].copy()
    mdl = pymf_amd.SIVM(data, num_bases=6)
    mdl.update_w()
    assert mdl.select == a["select"]
    v = a["select"][0]
    data.data[data.indptr[v]:data.indptr[v + 1]] = 0.0     # an in-place edit of the values: the first vertex becomes stored zeros
    mdl.update_w()
    want = ssc.so.update_w(data.toarray().astype(np.float64), 6)[0]
    assert want != a["select"] and mdl.select == want


def test_refusals_on_the_device():
    c = ssc.case("5x37_k3")
    ctx = _lib.Context(_lib.ALGO_SIVM, 5, 37, 3)
    try:
        bad = c["csc"].indices.copy()
        bad[0] = 5
        with pytest.raises(_lib.PmfError, match="row index out of range"):
            ctx.set_v_csc(c["csc"].indptr, bad, c["csc"].data)
        with pytest.raises(_lib.PmfError, match="CSR input is only wired"):
            ctx.set_v_csr(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
        ctx.set_option("sivm_sgreedy", 1)
        with pytest.raises(_lib.PmfError, match="SIVM_SGREEDY takes dense data only"):
            ctx.set_v_csc(c["csc"].indptr, c["csc"].indices, c["csc"].data)
    finally:
        ctx.close()
    nmf = _lib.Context(_lib.ALGO_NMF, 5, 37, 3)
    try:
        with pytest.raises(_lib.PmfError, match="SIVM contexts"):
            nmf.set_v_csc(c["csc"].indptr, c["csc"].indices, c["csc"].data)
    finally:
        nmf.close()
