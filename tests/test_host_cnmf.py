"""CPU-side checks of pymf_amd.CNMF: the reference's signature, its random draw, the refusals, and the argument checks of
the CNMF context (pmf_ctx_create with PMF_ALGO_CNMF).  No GPU needed."""
import inspect
import random

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib


def test_factorize_signature_and_argument_order_are_the_references():
    """cnmf.py:108-109: factorize(niter=10, compute_w=True, compute_h=True, compute_err=True, show_progress=False)."""
    sig = inspect.signature(pymf_amd.CNMF.factorize)
    params = list(sig.parameters.values())[1:]
    assert [p.name for p in params] == ["niter", "compute_w", "compute_h", "compute_err", "show_progress"]
    assert [p.default for p in params] == [10, True, True, True, False]
    init = inspect.signature(pymf_amd.CNMF.__init__)
    assert list(init.parameters)[1:] == ["data", "num_bases"] and init.parameters["num_bases"].default == 4


def test_cnmf_is_exported():
    assert "CNMF" in pymf_amd.__all__
    assert pymf_amd.CNMF._ALGO == _lib.ALGO_CNMF == 5


def test_hooks_are_noops_as_in_the_reference():
    mdl = pymf_amd.CNMF(np.ones((4, 3), dtype=np.float32), num_bases=2)
    assert mdl.update_w() is None and mdl.update_h() is None and mdl.init_w() is None
    assert not hasattr(mdl, "W") and not hasattr(mdl, "H") and not hasattr(mdl, "G")


def test_random_sample_is_called_once_with_the_references_arguments(monkeypatch):
    """kmeans.py:71: random.sample(xrange(n), k) on the global `random` -- once per initialisation, before any device work."""
    calls = []

    class Stop(Exception):
        pass

    def fake_sample(population, k):
        calls.append((list(population), k))
        raise Stop()

    monkeypatch.setattr(random, "sample", fake_sample)
    mdl = pymf_amd.CNMF(np.ones((5, 7), dtype=np.float32), num_bases=3)
    with pytest.raises(Stop):
        mdl.factorize(niter=2)
    assert calls == [(list(range(7)), 3)]


def test_random_sample_draw_matches_the_reference_stream(monkeypatch):
    """The indices drawn are exactly what kmeans.py:71 draws from a seeded global stream (the state it leaves included)."""
    seen = []
    real = random.sample

    def spy(population, k):
        out = real(population, k)
        seen.append(out)
        raise RuntimeError("stop")

    monkeypatch.setattr(random, "sample", spy)
    random.seed(11)
    with pytest.raises(RuntimeError):
        pymf_amd.CNMF(np.ones((5, 9), dtype=np.float32), num_bases=4).factorize()
    after = random.random()
    random.seed(11)
    expect = real(range(9), 4)
    assert seen == [expect] and random.random() == after


def test_h_without_g_raises_attribute_error():
    """cnmf.py:133-137: with H present init_h is skipped, and the loop's self.G raises AttributeError."""
    mdl = pymf_amd.CNMF(np.ones((4, 6), dtype=np.float32), num_bases=2)
    mdl.H = np.ones((2, 6))
    with pytest.raises(AttributeError):
        mdl.factorize(niter=1)


def test_sparse_data_is_refused():
    sp = pytest.importorskip("scipy.sparse")
    mdl = pymf_amd.CNMF(sp.random(20, 10, density=0.3, format="csr", random_state=1), num_bases=2)
    with pytest.raises(TypeError):
        mdl.factorize(niter=1)


def test_streamed_data_is_refused():
    mdl = pymf_amd.CNMF(np.ones((64, 8), dtype=np.float32), num_bases=2)
    mdl.stream_rows = 64
    with pytest.raises(ValueError):
        mdl.factorize(niter=1)


def test_multi_rank_world_is_refused(monkeypatch):
    class World(object):
        size, rank = 2, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    mdl = pymf_amd.CNMF(np.ones((8, 6), dtype=np.float32), num_bases=2)
    with pytest.raises(NotImplementedError):
        mdl.factorize(niter=1)


def _create_code(*args, **kw):
    try:
        _lib.Context(*args, **kw).close()
    except _lib.PmfError as e:
        return e.code
    return _lib.PMF_OK


def test_cnmf_context_limits():
    C = _lib.ALGO_CNMF
    assert _create_code(C, 64, 4097, 8) == _lib.PMF_EINVAL          # C = V^T V beyond 4096 samples
    assert _create_code(C, 64, 512, 129) == _lib.PMF_EINVAL         # num_bases > 128
    assert _create_code(C, 64, 10, 11) == _lib.PMF_EINVAL           # num_bases > n
    assert _create_code(C, 64, 512, 8, nranks=2, nccl_id=b"\0" * _lib.NCCL_ID_BYTES) == _lib.PMF_EINVAL
    assert _create_code(7, 4, 4, 2) == _lib.PMF_EINVAL              # algo 7 is still unknown


def test_cnmf_context_on_a_valid_shape_needs_the_device():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    assert _create_code(_lib.ALGO_CNMF, 300, 64, 6) == _lib.PMF_EHIP
    assert _create_code(_lib.ALGO_CNMF, 64, 4096, 128) == _lib.PMF_EHIP
