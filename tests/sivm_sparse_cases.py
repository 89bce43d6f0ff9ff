"""The device cases of SIVM and LAESA on scipy.sparse data (tests/test_gpu_sivm_sparse.py) and what makes the comparison with
the float64 oracle on toarray() meaningful (tests/test_sivm_sparse_cases.py, no GPU).

Data are planted and sparse: k vertices, vertex j a large entry (between `scale` and twice that, k > 16: three times) on a row
of its own (k <= m) and s - 1 smaller ones on random rows; every other column a convex mixture of three vertices (weights 0.6
Dirichlet(1) + 0.4 / 3, strictly inside) plus two stored noise entries of 3 % of `scale` on random rows.  All values are
float32-representable.  A seed is the first one at which, for the combination of rule, metric and init (a case's own seed: for
most of its combinations; SEEDS: for the others), every argmax keeps sivm_cases.MIN_GAP, the float32 sparse-form twin (sivm_sparse_oracle) selects what the
float64 oracle selects, and (H_CASES) W^T W stays below MAX_COND.
"""
import itertools

import numpy as np
import scipy.sparse as sp

import colsel_oracle as co
import sivm_cases as sc
import sivm_oracle as so
import sivm_sparse_oracle as sso

RULES = ("sivm", "laesa")
METRICS = ("l2", "l1", "cosine")
INITS = ("fastmap", "origin")
ALL = tuple(itertools.product(RULES, METRICS, INITS))
L2_ONLY = tuple((r, "l2", i) for r in RULES for i in INITS)

# name: (m, n, k, s, seed, special, the (rule, metric, init) combinations that run on it)
CASES = {
    "5x37_k3": (5, 37, 3, 2, 2, None, ALL),
    "29x300_k6": (29, 300, 6, 5, 5, None, ALL),
    "31x300_k6": (31, 300, 6, 5, 29, None, ALL),
    "64x4113_k8": (64, 4113, 8, 6, 1, "ends", ALL),                  # vertices in the first and in the last column
    "16384x1000_k6": (16384, 1000, 6, 40, 46, None, ALL),             # the row limit: x fills the 64 KiB of dynamic LDS
    "64x2048_k64": (64, 2048, 64, 4, 45, None, ALL),
    "16x640_k4_tie": (16, 640, 4, 4, 1, "tie", ALL),                 # columns 70 and 600 equal: the lower index wins
    "29x300_k6_empty": (29, 300, 6, 5, 1, "empty", ALL),             # empty columns, among them 0 (the fastmap start) and the last
}
# several 64-column panels per workgroup (sivm_cases.PANEL_CASES): selection only
PANEL_CASES = {
    "8x65600_k3": (8, 65600, 3, 3, 4, "ends", ALL),
    "8x1048592_k3": (8, 1048592, 3, 3, 1, "trip2", (("sivm", "l2", "fastmap"), ("laesa", "l2", "fastmap"))),
}
EMPTY_COLUMNS = (0, 1, 17, 64, 150, 298, 299)
# the cases whose H is compared on the device (one simplex QP per column in the oracle: the small ones, and the row limit)
H_CASES = ("5x37_k3", "29x300_k6", "31x300_k6", "29x300_k6_empty", "16384x1000_k6")

# A combination whose conditions do not hold at its case's seed (the tuple above) has a seed of its own: the first one from 1 on
# at which they hold for it (find_seed(name, combo)).  NO_SEED lists the combinations for which none of the first SEED_TRIES
# seeds does: they stay in the tables above, tests/test_sivm_sparse_cases.py shows for each that the search fails, and the device
# tests do not run them.
SEED_TRIES = 150
SEEDS = {
    ("29x300_k6", "sivm", "l2", "origin"): 1,
    ("29x300_k6", "laesa", "l2", "origin"): 1,
    ("29x300_k6", "laesa", "l1", "origin"): 1,
    ("16x640_k4_tie", "sivm", "cosine", "fastmap"): 2,
    ("16x640_k4_tie", "sivm", "cosine", "origin"): 4,
    ("16x640_k4_tie", "laesa", "cosine", "origin"): 4,
    ("64x4113_k8", "sivm", "l1", "origin"): 6,
    ("64x4113_k8", "sivm", "cosine", "fastmap"): 12,
    ("64x4113_k8", "sivm", "cosine", "origin"): 2,
    ("64x4113_k8", "laesa", "cosine", "fastmap"): 3,
    ("64x2048_k64", "sivm", "l1", "fastmap"): 4,
    ("64x2048_k64", "sivm", "l1", "origin"): 65,
    ("64x2048_k64", "laesa", "l2", "origin"): 47,
    ("64x2048_k64", "laesa", "l1", "fastmap"): 1,
    ("64x2048_k64", "laesa", "cosine", "fastmap"): 74,
    ("64x2048_k64", "laesa", "cosine", "origin"): 74,
    ("16384x1000_k6", "sivm", "l2", "origin"): 11,
    ("16384x1000_k6", "laesa", "l1", "origin"): 17,
}
# 63 recurrence rounds over 2 048 columns: under these four some argmax gap stays below MIN_GAP at every seed 1 .. 150
NO_SEED = (
    ("64x2048_k64", "sivm", "l2", "origin"),
    ("64x2048_k64", "sivm", "cosine", "fastmap"),
    ("64x2048_k64", "sivm", "cosine", "origin"),
    ("64x2048_k64", "laesa", "l1", "origin"),
)

# Worst relative Frobenius deviation of H, over H_CASES and their combinations, between the all-float64 oracle and the oracle with
# float32 V, W, right-hand sides and X (tests/test_sivm_sparse_cases.py re-measures it per case and holds it to this figure);
# the device tolerance is 4 x the worst: the margin the dense tests give for a different summation order.
#   2.62e-05 at 16384x1000_k6 under SIVM, 'l2', 'origin' (cond(W^T W) = 9.4e3); 1.53e-05 at 31x300_k6 under LAESA, 'l1', 'fastmap'
#   (cond 6.0e3), 1.12e-05 and 9.9e-06 at two more combinations of 31x300_k6 (cond 7.4e3, 8.4e3); below 4e-07 everywhere else
MEASURED_H_SPARSE = 2.62e-05
H_TOL = 4.0 * MEASURED_H_SPARSE

_cache = {}


def planted(m, n, k, s, seed, special=None, scale=4.0):
    """(csc float32 [m][n], vertex columns)"""
    rng = np.random.RandomState(seed)
    verts = np.zeros((m, k))
    own = rng.permutation(m)[:k] if k <= m else rng.randint(0, m, size=k)
    lengths = scale * rng.permutation(np.linspace(1.0, 3.0 if k > 16 else 2.0, k))
    if special == "tie":                                  # the longest vertex is the one that gets a twin
        lengths[[0, int(np.argmax(lengths))]] = lengths[[int(np.argmax(lengths)), 0]]
    for j in range(k):
        rows = rng.choice(m, size=min(s, m), replace=False)
        verts[rows, j] = 0.25 * lengths[j] * rng.uniform(0.2, 1.0, size=len(rows))
        verts[own[j], j] = lengths[j]
    three = np.argsort(rng.random_sample((n, k)), axis=1)[:, :3]
    weights = 0.6 * rng.dirichlet(np.ones(3), size=n) + 0.4 / 3.0
    V = np.zeros((m, n))
    for t in range(3):
        V += verts[:, three[:, t]] * weights[:, t]
    noise_rows = rng.randint(0, m, size=(n, 2))
    for t in range(2):
        V[noise_rows[:, t], np.arange(n)] += 0.03 * scale * rng.uniform(0.5, 1.0, size=n)
    cols = np.sort(rng.choice(np.arange(2, n - 2), size=k, replace=False))
    if special in ("ends", "trip2"):
        cols[0], cols[-1] = 3, n - 2
    if special == "trip2":
        cols[1] = sc.TRIP2_COLUMN
    if special == "tie":
        cols = np.array([70, 200, 333, 477])[:k]
    if special == "empty":
        cols = np.array([c for c in range(5, n - 5) if c not in EMPTY_COLUMNS])[rng.choice(n - 10 - 3, size=k, replace=False)]
        cols.sort()
    V[:, cols] = verts
    if special == "tie":
        V[:, 600] = V[:, 70]
    if special == "empty":
        V[:, list(EMPTY_COLUMNS)] = 0.0
    csc = sp.csc_matrix(V.astype(np.float32))
    csc.sort_indices()
    return csc, [int(c) for c in cols]


def _oracle(V64, k, rule, metric, init, scores):
    if rule == "sivm":
        return so.update_w(V64, k, metric, init, scores=scores)
    return co.laesa_update_w(V64, k, metric, init, scores=scores)


def spec(name):
    return CASES.get(name) or PANEL_CASES[name]


def seed_of(name, rule="sivm", metric="l2", init="fastmap"):
    return SEEDS.get((name, rule, metric, init), spec(name)[4])


def combos(table):
    """the (name, rule, metric, init) that run"""
    return [(name,) + combo for name in sorted(table) for combo in table[name][6] if (name,) + combo not in NO_SEED]


def data(name, seed=None):
    """(csc, dense float64 image, vertex columns) of a case at a seed (default: the case's own)"""
    seed = spec(name)[4] if seed is None else seed
    key = ("data", name, seed)
    if key not in _cache:
        m, n, k, s, _, special, _ = spec(name)
        csc, verts = planted(m, n, k, s, seed, special)
        _cache[key] = (csc, csc.toarray().astype(np.float64), verts)
    return _cache[key]


def case(name, rule="sivm", metric="l2", init="fastmap"):
    """dict(csc, V (dense float32), k, verts, special, select, W, scores): the float64 oracle on toarray()"""
    key = (name, rule, metric, init, seed_of(name, rule, metric, init))
    if key not in _cache:
        csc, V64, verts = data(name, key[4])
        k, special = spec(name)[2], spec(name)[5]
        scores = []
        select, W = _oracle(V64, k, rule, metric, init, scores)
        _cache[key] = dict(csc=csc, V=V64.astype(np.float32), k=k, verts=verts, special=special, select=select, W=W, scores=scores)
    return _cache[key]


def h_oracle(name, rule="sivm", metric="l2", init="fastmap"):
    """(H, ferr) of the float64 oracle for the case's W (sivm_oracle.update_h)"""
    key = ("H", name, rule, metric, init, seed_of(name, rule, metric, init))
    if key not in _cache:
        c = case(name, rule, metric, init)
        _cache[key] = so.update_h(c["V"].astype(np.float64), c["W"])
    return _cache[key]


def has_h(name, rule, metric, init):
    """Is H compared for this combination?  On H_CASES, both inits (seeds are chosen so that W^T W stays below MAX_COND under
    'origin' too, where the first column of W is the last data column, a mixture).  Not where there is no H: on the case with
    empty columns under 'origin' (-1 reads the empty last column: W has a zero column, W^T W is singular and update_h raises)
    and under 'cosine' (every cosine distance to the empty column 0 is exactly 1, column 0 is selected over and over)."""
    if name == "29x300_k6_empty" and (init == "origin" or metric == "cosine"):
        return False
    return name in H_CASES


def gap(scores, metric="l2", tie=False):
    """The smallest argmax gap of the steps, as a fraction of the scores' spread (max - median).  Scores that EQUAL the maximum
    are not runners-up where equality is exact on both sides: the planted twin columns (`tie`), and under 'cosine' the columns
    whose support is disjoint from every measured column's -- v.x is a sum of exact zeros there, the distance exactly 1 in
    float32 and in float64, and the lowest index wins on the device as in np.argmax."""
    worst = np.inf
    for s in scores:
        s = s[~np.isnan(s)]                               # (a NaN score never wins on the device; a seed at which the oracle's np.argmax picks one fails the twin test)
        o = np.sort(s)[::-1]
        below = o[o < o[0]] if (tie or metric == "cosine") else o[1:]
        if len(below):                                    # (none: every score the same bits -- cosine against the origin -- and column 0 wins)
            worst = min(worst, (o[0] - below[0]) / (o[0] - np.median(s)))
    return worst


def conditions(name, rule, metric, init):
    """(argmax gap, twin selects the oracle's selection, cond(W^T W) or None where W has a zero column)"""
    c = case(name, rule, metric, init)
    twin = sso.select32(c["csc"], c["k"], metric, init, rule)
    W = c["W"]
    cond = None if not np.all(np.abs(W).sum(axis=0) > 0) else float(np.linalg.cond(W.T.dot(W)))
    return gap(c["scores"], metric, c["special"] == "tie"), twin == c["select"], cond


def holds(name, rule, metric, init):
    """the conditions of one combination at its seed"""
    g, same, cond = conditions(name, rule, metric, init)
    c = case(name, rule, metric, init)
    ok = g >= sc.MIN_GAP and same and (not has_h(name, rule, metric, init) or cond <= sc.MAX_COND)
    if c["special"] == "tie":
        ok = ok and 70 in c["select"] and 600 not in c["select"]
    return bool(ok)


def find_seed(name, combo, start=1, tries=SEED_TRIES):
    """The first seed from `start` on at which the conditions hold for the combination (how the entries of SEEDS were chosen),
    or None."""
    key = (name,) + tuple(combo)
    had = SEEDS.get(key)
    try:
        for seed in range(start, start + tries):
            SEEDS[key] = seed
            if holds(*key):
                return seed
        return None
    finally:
        SEEDS.pop(key, None)
        if had is not None:
            SEEDS[key] = had
