"""pymf_amd.CHNMF without a GPU: the export, the signatures, the base_sel clipping, the refusals, and the order of the draws
(one np.random.randn(base_sel, rows) before anything else touches the stream), checked with a stand-in context."""
import inspect
import os
import re

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib
from pymf_amd import chnmf as mod
from conftest import ROOT


def test_export_and_signatures():
    assert pymf_amd.CHNMF is mod.CHNMF and "CHNMF" in pymf_amd.__all__ and mod.__all__ == ["CHNMF"]
    assert issubclass(pymf_amd.CHNMF, pymf_amd.AA)
    assert str(inspect.signature(pymf_amd.CHNMF.__init__)) == "(self, data, num_bases=4, base_sel=3)"
    assert str(inspect.signature(pymf_amd.CHNMF.factorize)) == \
        "(self, show_progress=False, compute_w=True, compute_h=True, compute_err=True, niter=1)"      # chnmf.py:193-194


def test_cabi_declares_and_binds_the_hull_entry():
    header = open(os.path.join(ROOT, "include", "pymf_hip.h")).read()
    assert re.search(r"int\s+pmf_chnmf_hull\(pmf_ctx\*\s*ctx,\s*const double\*\s*R,\s*int32_t\s+base_sel,\s*int32_t\*\s*idx_out,\s*"
                     r"int64_t\s+cap,\s*int64_t\*\s*count_out\);", header)
    bound = [s[0] for s in _lib.SYMBOLS]
    for name in ("pmf_chnmf_hull", "pmf_chnmf_set_limits", "pmf_chnmf_routes"):
        assert name in bound
    for name in ("chnmf_hull", "chnmf_set_limits", "chnmf_routes"):
        assert hasattr(_lib.Context, name)


def test_base_sel_is_clipped_to_the_rows():
    data = np.ones((5, 9), dtype=np.float32)
    assert pymf_amd.CHNMF(data, num_bases=2)._base_sel == 3
    assert pymf_amd.CHNMF(data, num_bases=2, base_sel=5)._base_sel == 5
    assert pymf_amd.CHNMF(data, num_bases=2, base_sel=40)._base_sel == 5             # chnmf.py:127-129
    assert pymf_amd.CHNMF(np.ones((2, 3)), num_bases=2)._base_sel == 2


def test_init_draws_nothing():
    mdl = pymf_amd.CHNMF(np.ones((5, 9), dtype=np.float32), num_bases=2)
    state = np.random.get_state()[1].copy()
    mdl.init_w()
    mdl.init_h()
    assert np.array_equal(np.random.get_state()[1], state)
    assert mdl.W.shape == (5, 2) and not mdl.W.any() and mdl.H.shape == (2, 9) and not mdl.H.any()     # chnmf.py:131-135


def test_refusals():
    import scipy.sparse as sp
    calls = [lambda m: m.factorize(), lambda m: m.update_w(), lambda m: m.update_h(), lambda m: m.frobenius_norm()]
    for call in calls:
        with pytest.raises(TypeError, match="scipy.sparse"):
            call(pymf_amd.CHNMF(sp.csr_matrix(np.ones((5, 9), dtype=np.float32)), num_bases=2))
        mdl = pymf_amd.CHNMF(np.ones((5, 9), dtype=np.float32), num_bases=2)
        mdl.stream_rows = 4
        with pytest.raises(ValueError, match="streamed"):
            call(mdl)
        with pytest.raises(ValueError, match="num_bases"):
            call(pymf_amd.CHNMF(np.ones((5, 90), dtype=np.float32), num_bases=65))
        with pytest.raises(ValueError, match="corral"):
            call(pymf_amd.CHNMF(np.ones((200, 300), dtype=np.float32), num_bases=4))
    for call in calls[:2]:
        with pytest.raises(ValueError, match="base_sel"):
            call(pymf_amd.CHNMF(np.ones((40, 90), dtype=np.float32), num_bases=2, base_sel=17))
        with pytest.raises(ValueError, match="base_sel"):
            call(pymf_amd.CHNMF(np.ones((1, 9), dtype=np.float32), num_bases=2))      # one row: no pair of projections


def test_multi_rank_world_is_refused(monkeypatch):
    class World(object):
        size, rank = 2, 0
    mdl = pymf_amd.CHNMF(np.ones((5, 9), dtype=np.float32), num_bases=2)
    monkeypatch.setattr(mdl, "_world", lambda: World())
    with pytest.raises(NotImplementedError, match="one rank"):
        mdl.factorize()


def test_update_w_draws_r_first_and_composes_the_reference(monkeypatch):
    """R = np.random.randn(base_sel, rows) is the first draw; the hull pass gets exactly that R; AA runs on data[:, _hull_idx]
    for 50 iterations; W is AA's; Wmapped holds the nearest data columns."""
    rs = np.random.RandomState(3)
    data = rs.random_sample((6, 40)).astype(np.float32)
    log = []

    class Ctx(object):
        def chnmf_hull(self, R):
            log.append(("hull", np.array(R)))
            return np.array([2, 5, 11, 30], dtype=np.int32)

    class FakeAA(object):
        def __init__(self, sub, num_bases=4):
            log.append(("aa", np.array(sub), num_bases, np.random.get_state()[1].copy()))
            self.data = sub

        def factorize(self, niter=1, show_progress=False, compute_w=True, compute_h=True, compute_err=True):
            log.append(("factorize", niter, compute_w, compute_h, compute_err))
            self.W = np.asarray(self.data[:, [3, 0]], dtype=np.float64) + 1e-3
            self.ferr = np.zeros(niter)

    mdl = pymf_amd.CHNMF(data, num_bases=2, base_sel=4)
    monkeypatch.setattr(mdl, "_sync_to_device", lambda *a, **k: Ctx())
    monkeypatch.setattr(mod, "AA", FakeAA)
    np.random.seed(99)
    mdl.update_w()
    np.random.seed(99)
    R = np.random.randn(4, 6)
    after_r = np.random.get_state()[1].copy()
    assert [e[0] for e in log] == ["hull", "aa", "factorize"]
    assert np.array_equal(log[0][1], R)
    assert np.array_equal(log[1][3], after_r)                  # nothing but R was drawn before the nested AA
    assert np.array_equal(log[1][1], data[:, [2, 5, 11, 30]]) and log[1][2] == 2
    assert log[2] == ("factorize", 50, True, True, True)
    assert mdl._hull_idx.dtype == np.int32 and list(mdl._hull_idx) == [2, 5, 11, 30]
    assert np.array_equal(mdl.W, data[:, [30, 2]].astype(np.float64) + 1e-3)
    assert list(mdl._Wmapped_index) == [30, 2] and np.array_equal(mdl.Wmapped, data[:, [30, 2]])
