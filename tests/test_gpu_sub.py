"""pymf_amd.SUB on the device: the composition equals the same steps done by hand with host slices and ordinary uploads (idx,
W, H and ferr[0] array_equal: the device paths are bit-identical from run to run, and a gathered V is the uploaded V), mapW
binds data columns, the full data cross the host link once per factorize(), and the reference's doctest-sized case."""
import random

import numpy as np
import pytest

import pymf_amd
import sub_cases as sc
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

MFMETHODS = ("NMF", "NMFALS", "Kmeans", "SIVM")
STRATEGIES = ("rand", "cur", "kmeans", "sivm", "laesa")
CUR_SEED = [s for (r, n, nsub, s) in sc.CUR_CASES if (r, n) == sc.COMPOSITION_SHAPE and nsub == sc.COMPOSITION["nsub"]][0]


def seed_all():
    random.seed(7)
    np.random.seed(CUR_SEED)


def select_by_hand(V, strategy, nsub):
    n = V.shape[1]
    if strategy == "rand":
        return random.sample(range(n), nsub)
    if strategy == "cur":
        _, pcol = pymf_amd.CUR(V).sample_probability()
        cum = np.cumsum(pcol.flatten())
        return [np.where(cum >= np.random.rand())[0][0] for _ in range(nsub)]
    if strategy == "kmeans":
        km = pymf_amd.Kmeans(V, num_bases=nsub)
        km.factorize()
        return pymf_amd.vq(km, km.W)
    cls = pymf_amd.SIVM if strategy == "sivm" else pymf_amd.LAESA
    sel = cls(V, num_bases=nsub, dist_measure="cosine")
    sel.factorize(compute_h=False, compute_err=False)
    return sel.select


@pytest.fixture(scope="module")
def V():
    return sc.sub_data(*sc.COMPOSITION_SHAPE)


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("name", MFMETHODS)
def test_composition_equals_the_steps_by_hand(name, strategy, V):
    """Random draws, in order, under random.seed(7) and np.random.seed(CUR_SEED) -- the same in SUB and in the replay:
      1. the strategy: 'rand' random.sample(range(n), nsub); 'kmeans' Kmeans.init_w's random.sample(range(n), nsub);
         'cur' nsub np.random.rand() draws; 'sivm' / 'laesa' none
      2. the small model's factorize(): NMF / NMFALS init_w then init_h from np.random (m x k, then k x nsub); Kmeans init_w
         from random.sample(range(nsub), k); SIVM none
      3. the full model's factorize(compute_w=False): NMF / NMFALS init_h from np.random (k x n); Kmeans and SIVM none"""
    cls = getattr(pymf_amd, name)
    nsub, k = sc.COMPOSITION["nsub"], sc.COMPOSITION["num_bases"]
    seed_all()
    sub = pymf_amd.SUB(V, cls, nsub=nsub, num_bases=k, sstrategy=strategy, show_progress=False)
    sub.factorize()
    seed_all()
    idx = np.sort(np.int32(select_by_hand(V, strategy, nsub)))
    small = cls(V[:, idx], num_bases=k)
    small.factorize()
    full = cls(V, num_bases=k)
    full.W = np.copy(small.W)
    full.factorize(niter=1, compute_w=False)
    assert np.array_equal(sub._idx, idx)
    assert np.array_equal(sub.W, full.W) and np.array_equal(sub.H, full.H)
    assert sub.ferr.shape == (1,) and sub.ferr[0] == full.frobenius_norm() and sub.ferr[0] == sub.mdl.frobenius_norm()
    assert np.array_equal(sub.W, sub.mdl.W) and sub.H.shape == (k, V.shape[1]) and np.all(np.isfinite(sub.H))
    if strategy == "cur":
        assert np.array_equal(idx, sc.cur_reference(V, nsub, CUR_SEED)[0])      # ... the float64 NumPy reference's indices


def test_mapw_binds_data_columns(V):
    nsub, k = sc.COMPOSITION["nsub"], sc.COMPOSITION["num_bases"]
    seed_all()
    sub = pymf_amd.SUB(V, pymf_amd.NMF, nsub=nsub, num_bases=k, mapW=True, show_progress=False)
    sub.factorize()
    seed_all()
    idx = np.sort(np.int32(random.sample(range(V.shape[1]), nsub)))
    small = pymf_amd.NMF(V[:, idx], num_bases=k)
    small.factorize()
    named = pymf_amd.vq(sub.mdl, np.asarray(small.W))
    assert named.shape == (k,)
    for j in range(k):
        assert np.array_equal(np.asarray(sub.W[:, j], dtype=np.float32).view(np.uint32), V[:, named[j]].view(np.uint32)), j


@pytest.fixture
def uploads(monkeypatch):
    counter = {"bytes": 0}
    real = _lib.Context.set_v_dense

    def counting(self, V):
        V = np.asarray(V)
        counter["bytes"] += int(V.shape[0]) * int(V.shape[1]) * 4
        return real(self, V)
    monkeypatch.setattr(_lib.Context, "set_v_dense", counting)
    return counter


@pytest.mark.parametrize("strategy", ["rand", "kmeans", "sivm"])
def test_the_full_data_go_up_once(strategy, uploads):
    V = sc.sub_data(*sc.UPLOAD_SHAPE)
    once = V.shape[0] * V.shape[1] * 4
    seed_all()
    sub = pymf_amd.SUB(V, pymf_amd.NMF, nsub=20, num_bases=4, sstrategy=strategy, show_progress=False)
    sub.factorize()
    assert uploads["bytes"] == once
    seed_all()
    sub.factorize()                                            # unchanged data: nothing more
    assert uploads["bytes"] == once
    W1, H1 = np.array(sub.W), np.array(sub.H)
    V[:, ::3] *= 0.25                                          # an in-place edit
    seed_all()
    sub.factorize()
    assert uploads["bytes"] == 2 * once
    seed_all()
    fresh = pymf_amd.SUB(V.copy(), pymf_amd.NMF, nsub=20, num_bases=4, sstrategy=strategy, show_progress=False)
    fresh.factorize()
    assert np.array_equal(sub.W, fresh.W) and np.array_equal(sub.H, fresh.H) and sub.ferr[0] == fresh.ferr[0]
    assert not np.array_equal(sub.H, H1)                       # the result reflects the edit


def test_doctest_sized_case():
    data = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
    np.random.seed(1)
    random.seed(1)
    with pytest.warns(pymf_amd.nmf.PrecisionWarning):
        sub = pymf_amd.SUB(data, pymf_amd.NMF, nsub=2, num_bases=2)
        sub.factorize()
    assert sub.W.shape == (2, 2) and sub.H.shape == (2, 3) and sub.ferr.shape == (1,)
    assert np.all(sub.W >= 0) and np.all(sub.H >= 0)
    assert sub.ferr[0] == sub.mdl.frobenius_norm() and np.isfinite(sub.ferr[0])
