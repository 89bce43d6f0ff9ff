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
    "31x300_k6": (31, 300, 6, 12, 0.0, 4.0, "l2", "fastmap", None),             # 3-row tail (seed 12: the checks hold at it)
    "64x4113_k8": (64, 4113, 8, 13, 0.0, 4.0, "l2", "fastmap", "ends"),
    "130x1000_k12": (130, 1000, 12, 14, 0.0, 4.0, "l2", "fastmap", None),
    "29x300_k6_offset1000": (29, 300, 6, 15, 1000.0, 400.0, "l2", "fastmap", None),
    "16x640_k4_tie": (16, 640, 4, 16, 0.0, 4.0, "l2", "fastmap", "tie"),
    "64x2048_k64": (64, 2048, 64, 2167, 0.0, 4.0, "l2", "fastmap", None),
}

# The panel ranges of k_sivm_pass: more 64-column panels than the launch has workgroups (PMF_CL_MAX_WGS = 1024), so that a
# workgroup owns several and c_begin / c_end are formed with panels_per_wg > 1; the vertices sit in the first and in the last
# workgroup.  8 x 65 600 is 1 025 panels, 2 per workgroup, 513 workgroups, the last one with a single panel (65 600 is a multiple
# of 64: no pad columns); a workgroup's 32 quads of columns still fit one trip of the quad loop.  8 x 1 048 592 is 16 385 panels,
# 17 per workgroup -- 272 quads, so threads 0 .. 15 take a second trip -- 964 workgroups, the last one with 14 panels, the last
# panel with 16 columns; one of its vertices is planted where only that second trip looks (TRIP2_COLUMN).  Only the selection and W are compared on the device, through SIVM.factorize(compute_h=False) and
# through pmf_sivm_select: the simplex H step over that many columns is not what these cases are for and its float32 deviation
# would replace MEASURED_H, so they have no H and no ferr, stay out of test_rounds_and_fp32_deviation and of test_parity, and
# their oracle is update_w alone.  (The cosine seed is the first from 61 on whose every argmax keeps MIN_GAP.)
PANEL_CASES = {
    "8x65600_k3_l2": (8, 65600, 3, 61, 0.0, 4.0, "l2", "fastmap", "ends"),
    "8x65600_k3_l1": (8, 65600, 3, 61, 0.0, 4.0, "l1", "fastmap", "ends"),
    "8x65600_k3_cosine": (8, 65600, 3, 63, 0.0, 4.0, "cosine", "fastmap", "ends"),
    "8x65600_k3_origin": (8, 65600, 3, 61, 0.0, 4.0, "l2", "origin", "ends"),
    "8x1048592_k3_l2": (8, 1048592, 3, 61, 0.0, 4.0, "l2", "fastmap", "trip2"),
}
TRIP2_COLUMN = 1029      # quad 257 of workgroup 0 when a workgroup owns 17 panels: a winner that only the second trip of the quad loop sees

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
    'trip2': as 'ends', and the second vertex at TRIP2_COLUMN; 'tie': the extreme column of the fastmap start duplicated at
    columns 70 and 600."""
    rng = np.random.RandomState(seed)
    Q = np.linalg.qr(rng.randn(max(m, k), max(m, k)))[0][:m, :k] if k <= m else rng.randn(m, k) / np.sqrt(m)
    verts = offset + scale * rng.permutation(np.linspace(1.0, 3.0 if k > 16 else 2.0, k)) * (Q + 0.15 * rng.randn(m, k) / np.sqrt(m))
    h = 0.8 * rng.dirichlet(np.full(k, 0.5), size=n).T + 0.2 / k
    V = verts.dot(h) + 0.03 * scale * rng.randn(m, n) / np.sqrt(m)
    cols = np.sort(rng.choice(np.arange(2, n - 2), size=k, replace=False))
    if special in ("ends", "trip2"):
        cols[0], cols[-1] = 3, n - 2
    if special == "trip2":
        cols[1] = TRIP2_COLUMN
    if special == "tie":
        cols = np.array([70, 200, 333, 477])[:k]
    V[:, cols] = verts
    V = V.astype(np.float32)
    if special == "tie":
        V[:, 600] = V[:, 70]
    return V, [int(c) for c in cols]


def case(name):
    """dict(V float32, k, metric, init, verts, select, W, H, ferr): the float64 oracle on the float32-representable data
    (H and ferr None for the PANEL_CASES)."""
    if name in _cache:
        return _cache[name]
    m, n, k, seed, offset, scale, metric, init, special = CASES.get(name) or PANEL_CASES[name]
    V, verts = planted(m, n, k, seed, offset, scale, special)
    V64 = V.astype(np.float64)
    scores = []
    select, W = so.update_w(V64, k, metric, init, scores=scores)
    H, ferr = so.update_h(V64, W) if name in CASES else (None, None)
    _cache[name] = dict(V=V, k=k, metric=metric, init=init, verts=verts, special=special, select=select, W=W, H=H, ferr=ferr,
                        scores=scores)
    return _cache[name]
