"""pymf_amd.SIVM_GSAT without a GPU: export, the C entries declared, bound and documented, init_w, the refusals with their
exception types before any device call, and the seeded draw sequence of the one-call walk."""
import inspect
import os
import re

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib
from pymf_amd import sivm_gsat as mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pmf_gsat_start", "pmf_gsat_walk", "pmf_gsat_probe_vec", "pmf_gsat_get_volumes", "pmf_gsat_get_d")


def test_class_surface():
    assert pymf_amd.SIVM_GSAT is mod.SIVM_GSAT and "SIVM_GSAT" in pymf_amd.__all__
    assert issubclass(pymf_amd.SIVM_GSAT, pymf_amd.SIVM) and not issubclass(pymf_amd.SIVM_SGREEDY, pymf_amd.SIVM_GSAT)
    for hook in ("init_w", "init_h", "online_update_w", "update_w", "update_h", "factorize", "frobenius_norm"):
        assert callable(getattr(pymf_amd.SIVM_GSAT, hook))
    assert pymf_amd.SIVM_GSAT._MAX_BASES == 64 and pymf_amd.SIVM_GSAT._ALGO == _lib.ALGO_SIVM
    assert inspect.signature(pymf_amd.SIVM_GSAT.__init__) == inspect.signature(pymf_amd.SIVM.__init__)
    assert list(inspect.signature(pymf_amd.SIVM_GSAT.factorize).parameters) == [
        "self", "show_progress", "compute_w", "compute_h", "compute_err", "niter"]                 # sivm_gsat.py:128-129
    assert "num_bases <= data_dimension + 1" in mod.__doc__ and "rounding noise" in mod.__doc__


def test_entries_are_declared_bound_and_documented():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_gsat_walk\(pmf_ctx\*\s*ctx,\s*const int64_t\*\s*idx,\s*int64_t n,\s*int32_t\*\s*slots_out\);", header)
    assert re.search(r"int\s+pmf_gsat_probe_vec\(pmf_ctx\*\s*ctx,\s*const float\*\s*vec,\s*int32_t\*\s*slot_out\);", header)
    bound = {s[0] for s in _lib.SYMBOLS}
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in ENTRIES:
        assert re.search(r"int\s+%s\(" % name, header), name
        assert name in bound, name
        assert name in doc, name
    assert '"sivm_gsat"' in header and "sivm_gsat" in doc and "SIVM_GSAT" in doc
    for method in ("gsat_start", "gsat_walk", "gsat_probe_vec", "gsat_get_volumes", "gsat_get_d"):
        assert callable(getattr(_lib.Context, method))
    for name in ("README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, name)) as f:
            assert "SIVM_GSAT" in f.read(), name


def test_init_w_selects_the_first_columns_as_a_list_and_copies_them():
    V = np.random.RandomState(5).random_sample((4, 9))
    mdl = pymf_amd.SIVM_GSAT(V, num_bases=3)
    mdl.init_w()
    assert type(mdl.select) is list and mdl.select == list(range(3))
    assert np.array_equal(mdl.W, V[:, :3]) and not np.shares_memory(mdl.W, V)
    mdl.select[1] = 7                                          # (the assignment the reference's range object refuses)
    assert mdl.select == [0, 7, 2]
    assert not hasattr(mdl, "V") and not hasattr(mdl, "_v") and not hasattr(mdl, "D")            # before the first probe


def no_device(*a, **k):
    raise AssertionError("a device call was made")


def calls(mdl):
    return (mdl.factorize, lambda: mdl.factorize(niter=3, compute_h=False, compute_err=False), mdl.update_w,
            lambda: mdl.online_update_w(np.ones(3)), mdl.update_h)


def test_refusals_come_with_their_types_before_any_device_call(monkeypatch):
    sp = pytest.importorskip("scipy.sparse")
    monkeypatch.setattr(_lib, "Context", no_device)

    class World(object):
        size, rank = 2, 0

    def streamed():
        m = pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2)
        m.stream_rows = 64
        return m

    def two_ranks():
        m = pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2)
        m._world = lambda: World()
        return m

    refusals = [
        (lambda: pymf_amd.SIVM_GSAT(sp.csr_matrix(np.ones((3, 5))), num_bases=2), TypeError),
        (streamed, ValueError),
        (two_ranks, NotImplementedError),
        (lambda: pymf_amd.SIVM_GSAT(np.ones((3, 100)), num_bases=65), ValueError),
        (lambda: pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2, dist_measure="cosine"), NotImplementedError),
        (lambda: pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2, dist_measure="kl"), NotImplementedError),
        (lambda: pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2, dist_measure="abs_cosine"), NotImplementedError),
        (lambda: pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2, dist_measure="weighted_abs_cosine"), NotImplementedError),
        (lambda: pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2, dist_measure="chebyshev"), ValueError),
    ]
    for make, exc in refusals:
        for i in range(len(calls(make()))):
            mdl = make()
            if i >= 2:                                         # the single hooks need a W, as in the reference
                mdl.select, mdl.W = list(range(mdl._num_bases)), np.ones((3, mdl._num_bases))
            with pytest.raises(exc):
                calls(mdl)[i]()
    with pytest.raises(NotImplementedError, match="cosine_distance cannot take"):
        pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2, dist_measure="cosine").factorize()
    for measure in ("l2", "l1"):
        pymf_amd.SIVM_GSAT(np.ones((3, 5)), num_bases=2, dist_measure=measure)._check_supported()


def test_one_call_walk_draws_what_single_update_w_calls_draw():
    """factorize(niter=N, compute_h=False, compute_err=False) takes its N indices in one draw; N update_w() calls take
    them one by one: the same indices, and the stream stands at the same place afterwards."""
    V = np.random.RandomState(1).random_sample((4, 300))
    N = 40

    def recorder(mdl, seen):
        def walk(idx):
            seen.extend(int(i) for i in idx)
            return np.full(len(idx), -1)
        mdl._walk = walk

    a, one_call = pymf_amd.SIVM_GSAT(V, num_bases=3), []
    recorder(a, one_call)
    np.random.seed(11)
    a.factorize(niter=N, compute_h=False, compute_err=False)
    after_a = np.random.random()

    b, single = pymf_amd.SIVM_GSAT(V, num_bases=3), []
    recorder(b, single)
    b.init_w()
    np.random.seed(11)
    for _ in range(N):
        b.update_w()
    after_b = np.random.random()

    np.random.seed(11)
    reference = [int(np.floor(np.random.random() * 300)) for _ in range(N)]                     # sivm_gsat.py:120
    assert one_call == single == reference and len(one_call) == N
    assert after_a == after_b
    assert a.select == list(range(3)) and not hasattr(a, "ferr")
