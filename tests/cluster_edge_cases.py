"""Kmeans / Cmeans cases beyond tests/test_gpu_cluster.py: more than one 64-column panel per workgroup (n > 65 536), data away
from the origin, tight clusters.  Data, float64 oracle results (tests/cluster_oracle.py) and the same runs with W and H
rounded to float32 after every step ("stored": what float32 storage alone costs) -- each computed once and shared by
tests/test_cluster_edge_cases.py (no GPU: the cases leave room for float32) and tests/test_gpu_cluster_edges.py."""
import collections
import functools

import numpy as np

import cluster_oracle as co

NITER = 3
Case = collections.namedtuple("Case", "m n k seed sigma offset")

# 1 025 panels: 2 per workgroup, 513 workgroups, the last one with one half-full panel; W of one tile / of two tiles.
# 2 050 panels: 3 per workgroup, 684 workgroups, the last one with one ragged panel, two 16-base tiles.
# (sigma: small enough that none of the n samples comes within 1e-4 of a tie between two of the k centres)
PANEL_CASES = [Case(8, 65570, 3, 5, 0.1, 0.0), Case(70, 65570, 5, 5, 0.1, 0.0), Case(8, 131190, 17, 5, 0.02, 0.0)]
# d^2 << ||v||^2: an offset (||v||^2 grows, d^2 stays) or tight clusters (d^2 shrinks)
CANCEL_CASES = [Case(48, 600, 8, 1, 0.1, 10.0), Case(48, 600, 8, 1, 0.1, 100.0), Case(48, 600, 8, 1, 0.01, 0.0),
                Case(48, 600, 8, 1, 0.001, 0.0), Case(48, 600, 8, 1, 0.001, 100.0), Case(37, 4100, 5, 337, 0.1, 10.0)]
# W - mu (mu: the float64 row means of the data) is compared up to here: float32 storage of W alone costs 8e-6 of it at 100
CENTRED_MAX_OFFSET = 10.0


def case_id(c):
    return "%dx%d-k%d-sigma%g-off%g" % (c.m, c.n, c.k, c.sigma, c.offset)


def r32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def data(c):
    """(V float32, W0): planted clusters moved by c.offset, the perturbed true centres rounded to float32 (the device
    stores W in float32: both sides start from the same numbers)."""
    V, W0, _ = co.blobs(c.m, c.n, c.k, c.seed, sigma=c.sigma, spread=0.2 * c.sigma)
    return frozen((V.astype(np.float64) + c.offset).astype(np.float32), r32(W0 + c.offset))


def row_mean(c):
    return data(c)[0].astype(np.float64).mean(axis=1, keepdims=True)


def random_h0(c):
    return np.random.RandomState(7).random_sample((c.k, c.n))


def _kmeans(c, rnd):
    V, W0 = data(c)
    Vd = V.astype(np.float64)
    st = {"gap": np.inf}

    def step_h(W, st):
        st["assigned"], H, g = co.kmeans_update_h(Vd, W)
        st["gap"] = min(st["gap"], g)
        return H

    H = step_h(W0, st)
    W, H, ferr = co._loop(Vd, W0.copy(), H, st, lambda W, H, st: rnd(co.kmeans_update_w(Vd, W, st["assigned"])), step_h,
                          NITER, True, True, True)
    return frozen(W, H, st["assigned"], ferr) + (st["gap"],)


def _cmeans(c, rnd, from_centres):
    V, W0 = data(c)
    Vd = V.astype(np.float64)
    H0 = rnd(co.cmeans_update_h(Vd, W0)) if from_centres else rnd(random_h0(c))
    return frozen(*co._loop(Vd, W0.copy(), H0, None, lambda W, H, st: rnd(co.cmeans_update_w(Vd, W, H)),
                            lambda W, st: rnd(co.cmeans_update_h(Vd, W)), NITER, True, True, True))


@functools.lru_cache(maxsize=None)
def kmeans_oracle(c, stored=False):
    """Kmeans.factorize(niter=3) from W0 -> (W, H, assigned, ferr, smallest gap (d2 - d1) / ||v|| of the run)."""
    return _kmeans(c, r32 if stored else (lambda x: x))


@functools.lru_cache(maxsize=None)
def cmeans_oracle(c, stored=False, from_centres=False):
    """Cmeans.factorize(niter=3) -> (W, H, ferr), from W0 and random_h0(c), or (from_centres) from the memberships of W0:
    update_h(), then factorize().  From a random H0 the centres collapse onto the mean and H is nearly uniform."""
    return _cmeans(c, r32 if stored else (lambda x: x), from_centres)


@functools.lru_cache(maxsize=None)
def cmeans_hook_oracle(c, stored=False):
    """Cmeans.update_h() from W0 -> H."""
    V, W0 = data(c)
    H = co.cmeans_update_h(V.astype(np.float64), W0)
    return frozen(r32(H) if stored else H)[0]


def small_clusters():
    """The data of test_small_clusters_keep_their_centre: centre 2 gets one sample, centre 3 none -> (V, W0)."""
    rs = np.random.RandomState(11)
    V = (0.1 * rs.randn(16, 40)).astype(np.float32)
    V[:, :20] += 1.0
    V[:, 7] = 10.0
    W0 = np.zeros((16, 4), dtype=np.float32)
    W0[:, 0] = 1.0
    W0[:, 2] = 9.75
    W0[:, 3] = -50.0
    W0 += (0.01 * rs.randn(16, 4)).astype(np.float32)
    return V, W0
