"""The device cases of SIVM_SGREEDY (tests/test_gpu_sgreedy.py) and what makes the comparison with the float64 oracle
(tests/sgreedy_oracle.py) meaningful (tests/test_sgreedy_cases.py, no GPU): the smallest shapes at which k_sgreedy_pass and
k_sgreedy_step can go wrong.  The data are sivm_cases.planted's: well-separated vertices among convex mixtures of them, so that
the exact greedy volume selection finds the vertices with a wide lead.  The tie duplicates a vertex that is NOT the start of
the selection at column TIE_COLUMN, so that the tied pair tops the argmax of a volume round (the start's duplicate would only
score zero).

Rows 29, 30, 31 and 32 are the four row tails of the distance loop; 130 rows pass 64; 300 columns leave a ragged last panel;
80 x 2048 at 64 bases runs t = 1 .. 63, every width of the quadratic form (1 .. 8 blocks of 8).  The PANEL_CASES are
sivm_cases' shapes (two panels per workgroup; the second trip of the quad loop), compared for selection and W only.
"""
import numpy as np

import sgreedy_oracle as sg
import sivm_cases as sc
import sivm_oracle as so

# name: (m, n, k, seed, metric, init, special)
CASES = {
    "sgreedy_5x37_k3": (5, 37, 3, 11, "l2", "fastmap", None),
    "sgreedy_29x300_k6_l2": (29, 300, 6, 12, "l2", "fastmap", None),          # 1-row tail
    "sgreedy_29x300_k6_l1": (29, 300, 6, 22, "l1", "fastmap", None),          # (the start alone is l1 / cosine)
    "sgreedy_29x300_k6_cosine": (29, 300, 6, 52, "cosine", "fastmap", None),
    "sgreedy_29x300_k6_origin": (29, 300, 6, 12, "l2", "origin", None),
    "sgreedy_30x300_k6": (30, 300, 6, 12, "l2", "fastmap", None),             # 2-row tail
    "sgreedy_31x300_k6": (31, 300, 6, 12, "l2", "fastmap", None),             # 3-row tail
    "sgreedy_32x300_k9": (32, 300, 9, 12, "l2", "fastmap", None),             # no tail; t = 8 fills the second block of the form
    "sgreedy_130x1000_k12": (130, 1000, 12, 14, "l2", "fastmap", None),       # m > 64
    "sgreedy_64x4113_k8": (64, 4113, 8, 13, "l2", "fastmap", "ends"),         # ragged last panel, winners in both end panels
    "sgreedy_16x640_k4_tie": (16, 640, 4, 16, "l2", "fastmap", "sgtie"),
    "sgreedy_80x2048_k64": (80, 2048, 64, 2167, "l2", "fastmap", "wide"),     # the base limit: t = 1 .. 63 (planted_wide)
}
PANEL_CASES = {
    "sgreedy_8x65600_k3": (8, 65600, 3, 61, "l2", "fastmap", "ends"),
    "sgreedy_8x1048592_k3": (8, 1048592, 3, 61, "l2", "fastmap", "trip2"),
}
TRIP2_COLUMN = sc.TRIP2_COLUMN
TIE_COLUMN = 600

# The winner of every round must lead the runner-up by at least GAP_FACTOR x the worst relative score difference between the
# float32 twin and the float64 oracle in that case (tests/test_sgreedy_cases.py measures and prints both).
GAP_FACTOR = 100.0

# Worst deviation, over all cases, of the twins from the all-float64 oracle; tests/test_sgreedy_cases.py re-measures them and
# holds them to these figures.  The device tolerances are 4 x the worst.  The twin of the selection is
# sgreedy_oracle.update_w_twin (squared distances formed in float32, the Schur form).  The H step is SIVM's and has two twins,
# of which the worse counts: the exact solver on float32 V, W, right-hand sides and X (sivm_oracle.update_h), and the restated
# multiplier search of the device (sivm_oracle.simplex_rounds on the same float32 operands), which stops at |sum x - 1| <= 1e-6
# as the device does -- on the 'origin' case, whose first vertex is an interior data column, that stopping rule is what H
# deviates by (2.0e-07 against 8.0e-08 from the roundings alone).
#   _v (relative):          2.740e-07 at sgreedy_130x1000_k12 (the longest float32 sums; 1.6e-07 at sgreedy_80x2048_k64, below 8.2e-08 elsewhere)
#   H (relative Frobenius): 2.026e-07 at sgreedy_29x300_k6_origin (3.3e-08 .. 4.6e-08 everywhere else)
#   ferr (relative):        7.663e-08 at sgreedy_5x37_k3 (below 1.4e-08 everywhere else)
MEASURED_V = 2.740e-07
MEASURED_H = 2.026e-07
MEASURED_FERR = 7.663e-08
V_TOL = 4.0 * MEASURED_V
H_TOL = 4.0 * MEASURED_H
FERR_TOL = 4.0 * MEASURED_FERR

_cache = {}


def spec(name):
    return CASES.get(name) or PANEL_CASES[name]


def planted_wide(m, n, k, seed):
    """sivm_cases.planted with every vertex well outside the others' hull, for the base limit: orthogonal directions of lengths
    8 .. 12, the mixtures 0.6 Dirichlet(1/2) + 0.4 barycentre, the same noise.  With sivm_cases' vertex lengths (4 .. 12) and
    mixtures (0.8 / 0.2) the winner's lead at 64 bases stays below 100 x the float32 twin's deviation at every seed tried
    (2167 .. 2173: 15 .. 70 x)."""
    rng = np.random.RandomState(seed)
    Q = np.linalg.qr(rng.randn(m, m))[0][:, :k]
    verts = 4.0 * rng.permutation(np.linspace(2.0, 3.0, k)) * Q
    h = 0.6 * rng.dirichlet(np.full(k, 0.5), size=n).T + 0.4 / k
    V = verts.dot(h) + 0.03 * 4.0 * rng.randn(m, n) / np.sqrt(m)
    cols = np.sort(rng.choice(np.arange(2, n - 2), size=k, replace=False))
    V[:, cols] = verts
    return V.astype(np.float32), [int(c) for c in cols]


def data(m, n, k, seed, special):
    """(V float32 [m][n], planted vertex columns)"""
    if special == "wide":
        return planted_wide(m, n, k, seed)
    V, verts = sc.planted(m, n, k, seed, 0.0, 4.0, special if special in ("ends", "trip2") else None)
    if special == "sgtie":
        start = sg.start(V.astype(np.float64), "l2", "fastmap")
        V[:, TIE_COLUMN] = V[:, [c for c in verts if c != start][0]]
    return V, verts


def case(name):
    """dict(V float32, k, metric, init, special, verts, select, picks, W, v, H, ferr, scores): the literal float64 oracle on the
    float32-representable data (H and ferr None for the PANEL_CASES)."""
    if name in _cache:
        return _cache[name]
    m, n, k, seed, metric, init, special = spec(name)
    V, verts = data(m, n, k, seed, special)
    V64 = V.astype(np.float64)
    scores = []
    select, W, v, picks = sg.update_w(V64, k, metric, init, scores=scores)
    H, ferr = so.update_h(V64, W) if name in CASES else (None, None)
    _cache[name] = dict(V=V, k=k, metric=metric, init=init, special=special, verts=verts, select=select, picks=picks, W=W, v=v,
                        H=H, ferr=ferr, scores=scores)
    return _cache[name]


def lead(s, special):
    """(best - runner-up) / best of one round's scores; at the planted tie the identical pair counts as one winner"""
    o = np.sort(s[~np.isnan(s)])[::-1]
    runner_up = o[2] if (special == "sgtie" and o[0] == o[1]) else o[1]
    return (o[0] - runner_up) / o[0]
