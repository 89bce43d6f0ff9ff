"""The device cases of LAESA and GMAP (tests/test_gpu_colsel.py) and what makes the comparison with the float64 oracle
(tests/colsel_oracle.py) meaningful (tests/test_colsel_cases.py, no GPU): the smallest shapes at which k_laesa_pass and
k_gmap_pass can go wrong.  The data are sivm_cases.planted's; for GMAP 'nmf' they are shifted non-negative (the method
measures angles to the all-ones direction; the base-limit case is the exception, see there), and GMAP's tie duplicates the column of largest norm -- the winner of its round
0 -- at column TIE_COLUMN instead of the fastmap extreme.

Seeds: sivm_cases' seed for the shape where every argmax of the oracle -- in float64 and with the fp32-formed quantities
rounded through float32 -- keeps MIN_GAP, both select alike, W^T W stays below MAX_COND and the case reaches what its row
says ('ends': winners in the first and in the last 64 columns; 'trip2': TRIP2_COLUMN selected; 'tie': the tied pair on top
of an argmax); otherwise the first seed upward that does.  Those that moved: see the comments in the table."""
import numpy as np

import colsel_oracle as co
import sivm_cases as sc
import sivm_oracle as so

# name: (rule, m, n, k, seed, metric (LAESA) or method (GMAP), init, special)
CASES = {
    "laesa_5x37_k3": ("laesa", 5, 37, 3, 11, "l2", "fastmap", None),                 # one row past the unroll
    "laesa_29x300_k6_l2": ("laesa", 29, 300, 6, 12, "l2", "fastmap", None),          # 1-row tail
    "laesa_29x300_k6_l1": ("laesa", 29, 300, 6, 22, "l1", "fastmap", None),
    "laesa_29x300_k6_cosine": ("laesa", 29, 300, 6, 52, "cosine", "fastmap", None),
    "laesa_29x300_k6_origin": ("laesa", 29, 300, 6, 12, "l2", "origin", None),
    "laesa_31x300_k6": ("laesa", 31, 300, 6, 12, "l2", "fastmap", None),             # 3-row tail
    "laesa_130x1000_k12": ("laesa", 130, 1000, 12, 14, "l2", "fastmap", None),       # 2-row tail, m > 64
    "laesa_64x4113_k8": ("laesa", 64, 4113, 8, 13, "l2", "fastmap", "ends"),         # ragged last panel
    "laesa_16x640_k4_tie": ("laesa", 16, 640, 4, 16, "l2", "fastmap", "tie"),
    "laesa_64x2048_k64": ("laesa", 64, 2048, 64, 2184, "l2", "fastmap", None),       # the base limit (2167 .. 2183: gaps 5e-05 .. 8e-04)
    "gmap_5x37_k3": ("gmap", 5, 37, 3, 11, "pca", None, None),
    "gmap_29x300_k6_pca": ("gmap", 29, 300, 6, 12, "pca", None, None),
    "gmap_29x300_k6_aa": ("gmap", 29, 300, 6, 12, "aa", None, None),
    "gmap_29x300_k6_nmf": ("gmap", 29, 300, 6, 12, "nmf", None, None),
    "gmap_31x300_k6": ("gmap", 31, 300, 6, 12, "pca", None, None),
    "gmap_130x1000_k12": ("gmap", 130, 1000, 12, 14, "pca", None, None),
    "gmap_64x4113_k8": ("gmap", 64, 4113, 8, 13, "pca", None, "ends"),
    "gmap_16x640_k4_tie": ("gmap", 16, 640, 4, 16, "pca", None, "tie"),
    "gmap_64x2048_k64": ("gmap", 64, 2048, 64, 2167, "nmf", None, "unshifted"),      # the base limit, see below
}
# GMAP at the base limit.  A selected column's estimate is not zeroed but multiplied by 1 - |c| with c = v.v / (|v| |v|), which
# is 0 or one unit in the last place by the luck of the rounding, in the reference as here; under 'pca' and 'aa' every round
# then multiplies it by |v| again, and on the planted data (vertex lengths 1 .. 3) the longest selected vertices overtake the
# unselected short ones after about 50 rounds: the float64 oracle itself re-selects columns, differently under float32
# operands, at every seed from 2167 to 2226.  The same happens under 'nmf' on the shifted data (all cosines near 1, factors
# near 0.05 and uneven).  'nmf' on the unshifted data has factors near 1 for every vertex and keeps MIN_GAP through all 64
# rounds; the kernel does not look at signs, so this is what the base-limit case uses.

# The panel ranges (sivm_cases.PANEL_CASES): 8 x 65 600 is 1 025 panels, 2 per workgroup; 8 x 1 048 592 is 16 385 panels, 17
# per workgroup, so that threads 0 .. 15 take a second trip of the quad loop, where TRIP2_COLUMN sits.  Selection and W only.
PANEL_CASES = {
    "laesa_8x65600_k3": ("laesa", 8, 65600, 3, 61, "l2", "fastmap", "ends"),
    "laesa_8x1048592_k3": ("laesa", 8, 1048592, 3, 61, "l2", "fastmap", "trip2"),
    "gmap_8x65600_k3": ("gmap", 8, 65600, 3, 61, "pca", None, "ends"),
    "gmap_8x1048592_k3": ("gmap", 8, 1048592, 3, 61, "pca", None, "trip2"),
}
TRIP2_COLUMN = sc.TRIP2_COLUMN
TIE_COLUMN = 600

# Worst deviation, over all cases, between the all-float64 oracle and the oracle with float32 V, W, right-hand sides and X
# (tests/test_colsel_cases.py re-measures them per case and holds them to these figures); the tolerances of the device
# comparison are 4 x the worst, the project's rule (sivm_cases.py).
#   H (relative Frobenius): 1.108e-06 at gmap_29x300_k6_nmf (the shifted data: W^T v large against the vertex distances;
#                           4.2e-07 at gmap_64x2048_k64, 8.0e-08 at laesa_29x300_k6_origin, 3.0e-08 .. 3.7e-08 everywhere else)
#   ferr (relative):        6.376e-08 at laesa_5x37_k3 and gmap_5x37_k3 (1.3e-08 at gmap_29x300_k6_nmf, below 6e-09 everywhere else)
MEASURED_H = 1.108e-06
MEASURED_FERR = 6.376e-08
H_TOL = 4.0 * MEASURED_H
FERR_TOL = 4.0 * MEASURED_FERR

MIN_GAP = sc.MIN_GAP
MAX_COND = sc.MAX_COND

_cache = {}


def spec(name):
    return CASES.get(name) or PANEL_CASES[name]


def data(rule, m, n, k, seed, what, special):
    """(V float32 [m][n], planted vertex columns)"""
    gmap_tie = rule == "gmap" and special == "tie"
    V, verts = sc.planted(m, n, k, seed, 0.0, 4.0, special if special in ("ends", "trip2") or (special == "tie" and not gmap_tie) else None)
    if rule == "gmap" and what == "nmf" and special != "unshifted":
        V = V - V.min()
    if gmap_tie:
        V[:, TIE_COLUMN] = V[:, int(np.argmax((V.astype(np.float64) ** 2).sum(axis=0)))]
    return V, verts


def oracle(name, V, f32_ops=False, scores=None):
    rule, _, _, k, _, what, init, _ = spec(name)
    if rule == "laesa":
        return co.laesa_update_w(V, k, what, init, scores=scores, f32_ops=f32_ops)
    return co.gmap_update_w(V, k, what, scores=scores, f32_ops=f32_ops)


def case(name):
    """dict(V float32, rule, k, what, init, special, verts, select, W, H, ferr, scores): the float64 oracle on the
    float32-representable data (H and ferr None for the PANEL_CASES)."""
    if name in _cache:
        return _cache[name]
    rule, m, n, k, seed, what, init, special = spec(name)
    V, verts = data(rule, m, n, k, seed, what, special)
    V64 = V.astype(np.float64)
    scores = []
    select, W = oracle(name, V64, scores=scores)
    H, ferr = so.update_h(V64, W) if name in CASES else (None, None)
    _cache[name] = dict(V=V, rule=rule, k=k, what=what, init=init, special=special, verts=verts, select=select, W=W, H=H,
                        ferr=ferr, scores=scores)
    return _cache[name]


def gaps(scores, special):
    """per argmax: (best - runner-up) / (best - median); at a planted tie the gap to the third"""
    out = []
    for s in scores:
        s = s[~np.isnan(s)]
        o = np.sort(s)[::-1]
        runner_up = o[2] if (special == "tie" and o[0] == o[1]) else o[1]
        out.append((o[0] - runner_up) / (o[0] - np.median(s)))
    return out
