"""The device cases of SIVM (tests/test_gpu_sivm.py) and what makes the comparison with the float64 oracle meaningful
(tests/test_sivm_cases.py, no GPU): the smallest shapes at which the kernels can go wrong.

Data are planted: k well-separated vertices (random directions of lengths
between `scale` and twice (k > 16: three times) that, moved by `offset`) at random columns, every
other column a convex mixture of them with weights that keep it strictly inside (0.8 Dirichlet(1/2) + 0.2 barycentre), plus
Gaussian noise of 3 % of `scale` so that the fit is not exact and some columns leave the simplex (active constraints in the H
step).  All values are float32-representable.  The oracle's selection is then the set of planted vertices.
"""
import numpy as np

import sivm_oracle as so

# name: (m, n, k, seed, offset, scale, metric, init, special)
CASES = {
    "5x37_k3": (5, 37, 3, 11, 0.0, 4.0, "l2", "fastmap", None),
    "29x300_k6_l2": (29, 300, 6, 12, 0.0, 4.0, "l2", "fastmap", None),
    "29x300_k6_l1": (29, 300, 6, 22, 0.0, 4.0, "l1", "fastmap", None),
    "29x300_k6_cosine": (29, 300, 6, 52, 0.0, 4.0, "cosine", "fastmap", None),
    "29x300_k6_origin": (29, 300, 6, 12, 0.0, 4.0, "l2", "origin", None),
    "64x4113_k8": (64, 4113, 8, 13, 0.0, 4.0, "l2", "fastmap", "ends"),
    "130x1000_k12": (130, 1000, 12, 14, 0.0, 4.0, "l2", "fastmap", None),
    "29x300_k6_offset1000": (29, 300, 6, 15, 1000.0, 400.0, "l2", "fastmap", None),
    "16x640_k4_tie": (16, 640, 4, 16, 0.0, 4.0, "l2", "fastmap", "tie"),
    "64x2048_k64": (64, 2048, 64, 2167, 0.0, 4.0, "l2", "fastmap", None),
}

# Worst deviation, over all cases, between the all-float64 oracle and the oracle with float32 V, W, right-hand sides and X
# (tests/test_sivm_cases.py re-measures them per case and holds them to these figures); the tolerances of the device
# comparison are 4 x the worst, to leave room for a different summation order on the device.
#   H (relative Frobenius): 7.69e-06 at 29x300_k6_offset1000 (W^T v ~ 3e7 rounded to float32 against vertex distances ~ 6e2;
#                           7.6e-07 at 29x300_k6_origin, 3.2e-08 .. 3.6e-08 everywhere else)
#   ferr (relative):        6.38e-08 at 5x37_k3 (2.1e-08 at 29x300_k6_offset1000, below 2e-09 everywhere else)
MEASURED_H = 7.69e-06
MEASURED_FERR = 6.38e-08
H_TOL = 4.0 * MEASURED_H
FERR_TOL = 4.0 * MEASURED_FERR

ROUND_CAP = 48           # PMF_SIVM_ROUND_CAP (pymf_amd/csrc/pmf_host_sivm.h)
MIN_GAP = 1e-3           # argmax gap, as a fraction of the scores' spread (max - median)
MAX_COND = 1e4

_cache = {}


def planted(m, n, k, seed, offset=0.0, scale=4.0, special=None):
    """(V float32 [m][n], vertex columns).  special 'ends': vertices planted in the first and in the last 64 columns;
    'tie': the extreme column of the fastmap start duplicated at columns 70 and 600."""
    rng = np.random.RandomState(seed)
    Q = np.linalg.qr(rng.randn(max(m, k), max(m, k)))[0][:m, :k] if k <= m else rng.randn(m, k) / np.sqrt(m)
    verts = offset + scale * rng.permutation(np.linspace(1.0, 3.0 if k > 16 else 2.0, k)) * (Q + 0.15 * rng.randn(m, k) / np.sqrt(m))
    h = 0.8 * rng.dirichlet(np.full(k, 0.5), size=n).T + 0.2 / k
    V = verts.dot(h) + 0.03 * scale * rng.randn(m, n) / np.sqrt(m)
    cols = np.sort(rng.choice(np.arange(2, n - 2), size=k, replace=False))
    if special == "ends":
        cols[0], cols[-1] = 3, n - 2
    if special == "tie":
        cols = np.array([70, 200, 333, 477])[:k]
    V[:, cols] = verts
    V = V.astype(np.float32)
    if special == "tie":
        V[:, 600] = V[:, 70]
    return V, [int(c) for c in cols]


def case(name):
    """dict(V float32, k, metric, init, verts, select, W, H, ferr): the float64 oracle on the float32-representable data."""
    if name in _cache:
        return _cache[name]
    m, n, k, seed, offset, scale, metric, init, special = CASES[name]
    V, verts = planted(m, n, k, seed, offset, scale, special)
    V64 = V.astype(np.float64)
    scores = []
    select, W = so.update_w(V64, k, metric, init, scores=scores)
    H, ferr = so.update_h(V64, W)
    _cache[name] = dict(V=V, k=k, metric=metric, init=init, verts=verts, special=special, select=select, W=W, H=H, ferr=ferr,
                        scores=scores)
    return _cache[name]
