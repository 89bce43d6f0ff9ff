"""CPU-side checks of pymf_amd.Kmeans / pymf_amd.Cmeans: the exports, the reference's random draw, the refusals and the
argument checks of the contexts (pmf_ctx_create with PMF_ALGO_KMEANS / PMF_ALGO_CMEANS).  No GPU needed."""
import inspect
import random

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

CLASSES = ["Kmeans", "Cmeans"]


def test_classes_are_exported():
    assert "Kmeans" in pymf_amd.__all__ and "Cmeans" in pymf_amd.__all__
    assert pymf_amd.Kmeans._ALGO == _lib.ALGO_KMEANS == 6
    assert pymf_amd.Cmeans._ALGO == _lib.ALGO_CMEANS == 8      # (7 stays unassigned: pmf_ctx_create refuses it)
    assert issubclass(pymf_amd.Kmeans, pymf_amd.NMF) and issubclass(pymf_amd.Cmeans, pymf_amd.NMF)


@pytest.mark.parametrize("cls", CLASSES)
def test_factorize_signature_is_nmfs(cls):
    """Neither reference class overrides factorize: nmf.py:141-142."""
    assert inspect.signature(getattr(pymf_amd, cls).factorize) == inspect.signature(pymf_amd.NMF.factorize)


def test_kmeans_init_w_draws_the_references_sample():
    """kmeans.py:69-72: random.sample(xrange(n), k) on the global stream, sorted, W = data[:, sel]; the state it leaves."""
    data = np.random.RandomState(3).random_sample((5, 9)).astype(np.float32)
    random.seed(11)
    mdl = pymf_amd.Kmeans(data, num_bases=4)
    mdl.init_w()
    after = random.random()
    random.seed(11)
    sel = random.sample(range(9), 4)
    assert random.random() == after
    assert np.array_equal(mdl.W, data[:, np.sort(sel)])


def test_kmeans_draws_what_cnmf_draws():
    """The same call, the same stream state as pymf_amd/cnmf.py (CNMF.init_h)."""
    seen = []
    real = random.sample

    def spy(population, k):
        seen.append((list(population), k))
        return real(population, k)

    random.seed(5)
    try:
        random.sample = spy
        pymf_amd.Kmeans(np.ones((5, 7), dtype=np.float32), num_bases=3).init_w()
    finally:
        random.sample = real
    assert seen == [(list(range(7)), 3)]


def test_kmeans_update_w_without_an_assignment_raises_attribute_error():
    mdl = pymf_amd.Kmeans(np.ones((4, 6), dtype=np.float32), num_bases=2)
    mdl.W = np.ones((4, 2))
    mdl.H = np.ones((2, 6))
    with pytest.raises(AttributeError):
        mdl.update_w()
    with pytest.raises(AttributeError):
        mdl.factorize(niter=1)
    with pytest.raises(AttributeError):
        mdl.assigned


@pytest.mark.parametrize("cls", CLASSES)
def test_sparse_data_is_refused(cls):
    sp = pytest.importorskip("scipy.sparse")
    mdl = getattr(pymf_amd, cls)(sp.random(20, 10, density=0.3, format="csr", random_state=1), num_bases=2)
    with pytest.raises(TypeError):
        mdl.factorize(niter=1)


@pytest.mark.parametrize("cls", CLASSES)
def test_streamed_data_is_refused(cls):
    mdl = getattr(pymf_amd, cls)(np.ones((64, 8), dtype=np.float32), num_bases=2)
    mdl.stream_rows = 64
    with pytest.raises(ValueError):
        mdl.factorize(niter=1)


@pytest.mark.parametrize("cls", CLASSES)
def test_multi_rank_world_is_refused(cls, monkeypatch):
    class World(object):
        size, rank = 2, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    mdl = getattr(pymf_amd, cls)(np.ones((8, 6), dtype=np.float32), num_bases=2)
    with pytest.raises(NotImplementedError):
        mdl.factorize(niter=1)


@pytest.mark.parametrize("cls", CLASSES)
def test_more_than_128_bases_are_refused(cls):
    mdl = getattr(pymf_amd, cls)(np.ones((8, 300), dtype=np.float32), num_bases=129)
    with pytest.raises(ValueError):
        mdl.factorize(niter=1)
    for hook in (mdl.update_w, mdl.update_h, mdl.frobenius_norm):
        with pytest.raises(ValueError):
            hook()


def _create_code(*args, **kw):
    try:
        _lib.Context(*args, **kw).close()
    except _lib.PmfError as e:
        return e.code
    return _lib.PMF_OK


@pytest.mark.parametrize("algo", [6, 8])
def test_context_limits(algo):
    assert _create_code(algo, 64, 512, 129) == _lib.PMF_EINVAL
    assert _create_code(algo, 64, 512, 8, nranks=2, nccl_id=b"\0" * _lib.NCCL_ID_BYTES) == _lib.PMF_EINVAL
    assert _create_code(7, 4, 4, 2) == _lib.PMF_EINVAL and _create_code(9, 4, 4, 2) == _lib.PMF_EINVAL   # unassigned
