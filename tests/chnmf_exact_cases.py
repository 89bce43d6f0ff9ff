"""CHNMF hull cases whose answer is exact integer geometry (tests/test_chnmf_exact_cases.py, no GPU; tests/test_gpu_chnmf_exact.py
on the device).

The fixtures of tests/chnmf_cases.py keep every point 1e4 gamma away from every decision, because the device sums proj = R V in
another order than NumPy.  Here the projection itself is exact: R and V hold small integers, so every product and every partial
sum of R V is an integer below 2^53, the same in any summation order, fused or not.  The projected points are integers, every
cross product of the filter and of the chain is exact, and the expected `_hull_idx` is the mathematically exact strict hull,
computed below with Python integers: it does not depend on which extremes the filter picks or which route a pair takes.

build(targets, m, seed) makes (V, R) with R V == targets: R = [I | R2], R2 random integers in [-8, 8], the lower rows V2 of V
random integers in [-3, 3], the upper rows V1 = targets - R2 V2; for m == base_sel R is a signed permutation.  It asserts
|V| <= 2^24 (the float32 integers; the parabola's last point 4096^2 = 2^24 is among them), that V round-trips through float32
and that sum_r |R| |V| < 2^53 per entry.

Nothing here imports the library or needs a GPU."""
import itertools

import numpy as np

CAP = 4096                # PMF_CH_CAP (tests/test_chnmf_cases.py holds chnmf_cases.CAP to the header)
LIMIT = 2 ** 53


# ---- the exact oracle
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def exact_hull(x, y):
    """The sample indices of the strict convex-hull vertices of the integer points (x[q], y[q]), counter-clockwise from the lowest
    (x, y): monotone chain over Python ints, strict turn test (a point on an edge is no vertex), bit-identical points taken
    once, at their lowest index."""
    first = {}
    for q, p in enumerate(zip(np.asarray(x).tolist(), np.asarray(y).tolist())):
        assert isinstance(p[0], int) and isinstance(p[1], int)
        first.setdefault(p, q)
    order = sorted(first)
    if len(order) == 1:
        return [first[order[0]]]

    def chain(seq):
        st = []
        for p in seq:
            while len(st) >= 2 and _cross(st[-2], st[-1], p) <= 0:
                st.pop()
            st.append(p)
        return st
    return [first[p] for p in chain(order)[:-1] + chain(order[::-1])[:-1]]


def exact_union(P):
    """_hull_idx: the sorted union of exact_hull over all pairs of rows of the integer array P [base_sel][n], int32."""
    P = np.asarray(P)
    assert P.dtype == np.int64
    found = set()
    for i, j in itertools.combinations(range(P.shape[0]), 2):
        found.update(exact_hull(P[i], P[j]))
    return np.array(sorted(found), dtype=np.int32)


# ---- (V, R) with R V == targets exactly
def build(targets, m, seed):
    T = np.asarray(targets)
    assert T.dtype == np.int64 and T.ndim == 2
    s, n = T.shape
    assert 2 <= s <= m
    rng = np.random.RandomState(seed)
    if m == s:
        R = np.zeros((s, m), dtype=np.int64)
        R[np.arange(s), rng.permutation(s)] = rng.choice([-1, 1], size=s)
        V = R.T.dot(T)                                              # (a signed permutation: R R^T = I)
    else:
        R2 = rng.randint(-8, 9, size=(s, m - s)).astype(np.int64)
        V2 = rng.randint(-3, 4, size=(m - s, n)).astype(np.int64)
        R = np.hstack([np.eye(s, dtype=np.int64), R2])
        V = np.vstack([T - R2.dot(V2), V2])
    assert np.array_equal(R.dot(V), T)
    assert int(np.abs(V).max()) <= 2 ** 24
    V32 = V.astype(np.float32)
    assert np.array_equal(V32.astype(np.int64), V)
    assert int(np.abs(R).dot(np.abs(V)).max()) < LIMIT
    return V32, R.astype(np.float64)


# ---- the figures: int64 targets [base_sel][n]
def _shuffled(T, seed):
    T = np.asarray(T, dtype=np.int64)
    return np.ascontiguousarray(T[:, np.random.RandomState(seed).permutation(T.shape[1])])


def identical(n, seed):
    return np.array([[7] * n, [-3] * n], dtype=np.int64)


def two_points(n, seed):
    """B first, so that A's lowest index is not column 0; both repeated, interleaved"""
    pick = np.array([1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1][:n])
    return np.array([[-4, 9], [1, 6]], dtype=np.int64)[:, pick]


def line(n, seed, kind):
    """n - 4 distinct points t = 0 .. n - 5 on one line and two further copies of each endpoint, all in shuffled order (the copies
    of an endpoint are not in memory order of anything; the vertex is the lowest of the three indices)"""
    t = np.concatenate([np.arange(n - 4), [0, 0, n - 5, n - 5]]).astype(np.int64)
    t = t[np.random.RandomState(seed).permutation(n)]
    if kind == "horizontal":
        return np.stack([t - 20, np.full(n, 4, dtype=np.int64)])
    if kind == "vertical":
        return np.stack([np.full(n, -4, dtype=np.int64), t - 20])
    return np.stack([7 * t - 100, 3 * t + 11])                     # slope 3 / 7


def three_collinear(n, seed):
    return np.array([[7, 14, 0], [3, 6, 0]], dtype=np.int64)        # the middle point first: the hull is columns 1 and 2


def _grid(w, h):
    c = np.arange(w * h, dtype=np.int64)
    return np.stack([c % w - w // 2, c // w - h // 2])


def grid(n, seed, w):
    return _shuffled(_grid(w, w), seed)


def grid_dup_corners(n, seed, w):
    """every corner three times: the grid's own and two copies, all columns shuffled, so that a corner's lowest index is a
    copy's as often as the grid's own"""
    g = _grid(w, w)
    corners = g[:, [0, w - 1, w * (w - 1), w * w - 1]]
    return _shuffled(np.hstack([corners, g, corners]), seed)


def circle(n, seed, r):
    """every lattice point of the closed disc of radius r: those on the circle are in convex position, the rest inside or on
    the edges between them"""
    a = np.arange(-r, r + 1, dtype=np.int64)
    X, Y = np.meshgrid(a, a)
    inside = X * X + Y * Y <= r * r
    return _shuffled(np.stack([X[inside], Y[inside]]), seed)


DUP_COLUMNS = {"A": (63, 64, 2000, 4500), "B": (255, 256, 3000), "C": (1727, 1728, 4000), "D": (4991, 4999)}
DUP_SIDE = 1000


def dup_boundaries(n, seed):
    """A square's corners as copies at the columns of DUP_COLUMNS: across a wave (63 / 64), a 256-column trip (255 / 256), the
    27-panel boundary of max_wgs = 3 (1727 / 1728), the last full panel and the last column before the pad (4991 / 4999), further
    copies at higher indices only.  Every 97th other column lies on an edge of the square, the rest strictly inside.  Rows x, y
    and x + y: the third row shears the square, the corners stay the vertices of all three pairs."""
    assert n == 5000
    S = DUP_SIDE
    rng = np.random.RandomState(seed)
    x, y = rng.randint(1, S, size=n).astype(np.int64), rng.randint(1, S, size=n).astype(np.int64)
    y[::97] = 0
    x[50::97] = S
    for name, (cx, cy) in (("A", (0, 0)), ("B", (S, 0)), ("C", (S, S)), ("D", (0, S))):
        for c in DUP_COLUMNS[name]:
            x[c], y[c] = cx, cy
    return np.stack([x, y, x + y])


def parabola(n, seed):
    """(c, c^2, -c^2), c < n, shuffled: every column is a vertex of the pairs (0, 1) and (0, 2) -- lower and upper chains -- and
    pair (1, 2) is a line; all n points survive any filter in all three pairs"""
    c = np.arange(n, dtype=np.int64)
    return _shuffled(np.stack([c, c * c, -c * c]), seed)


def over_cap_vertex(n, seed):
    """a triangle, one vertex n - 100 times, 98 interior points: 30 of them first, the rest shuffled, so that the run's lowest
    index is not column 0"""
    rng = np.random.RandomState(seed)
    x = np.concatenate([np.full(n - 100, -50), [60, 0], rng.randint(-10, 11, size=98)]).astype(np.int64)
    y = np.concatenate([np.full(n - 100, -40), [-35, 70], rng.randint(-10, 11, size=98)]).astype(np.int64)
    T = np.stack([x, y])
    return np.hstack([T[:, -30:], _shuffled(T[:, :-30], seed + 1)])


def proj_figure(n, seed, rows=4):
    """a parabola in rows 0 / 1 (centred: at n = 4160 its squares stay float32 integers) and a partly filled grid in rows 2 / 3"""
    c = np.arange(n, dtype=np.int64)
    w = int(np.ceil(np.sqrt(n)))
    return _shuffled(np.stack([c - n // 2, (c - n // 2) ** 2, c % w, c // w])[:rows], seed)


def rows16(n, seed):
    """one distinct integer figure per row, 120 pairs"""
    c = np.arange(n, dtype=np.int64)
    rng = np.random.RandomState(seed)
    ang = 2.0 * np.pi * c / n
    rows = [c, c * c, -c * c, c % 33, c // 33, (c * c) % 97, np.abs(c - 530), rng.randint(-50, 51, size=n), rng.randint(-3, 4, size=n),
            np.rint(1000 * np.cos(ang)), np.rint(1000 * np.sin(ang)), c % 2, (7 * c) % 64, np.minimum(c, 500), np.full(n, 5),
            (c * c * c) % 1009]
    return _shuffled(np.stack([np.asarray(r).astype(np.int64) for r in rows]), seed + 1)


PANEL_CORNERS = (5, 40, 65560, 65599)


def panel_corners(n, seed):
    """a square's corners in the first and the last 64 columns, every other point strictly inside"""
    rng = np.random.RandomState(seed)
    x, y = rng.randint(1, 1000, size=n).astype(np.int64), rng.randint(1, 1000, size=n).astype(np.int64)
    for c, (cx, cy) in zip(PANEL_CORNERS, ((0, 0), (1000, 1000), (1000, 0), (0, 1000))):
        x[c], y[c] = cx, cy
    return np.stack([x, y])


# name: (figure, its arguments before the seed, m, n, seed, max_wgs values (0: the build's), forced routes or None)
#   routes: "device" -- every pair ends on the 32-direction filter and the device chain; "host" -- every pair on the host
CASES = {
    # degenerate sets: k_hull_polygon with no edge at all (one distinct point), with two, and with every edge on one line
    "identical_n1": (identical, (), 2, 1, 1, (0,), None),
    "identical_n2": (identical, (), 2, 2, 1, (0,), None),
    "identical_n64": (identical, (), 3, 64, 1, (0,), None),                       # one full panel, no pad column
    "identical_n300": (identical, (), 5, 300, 1, (0,), None),                     # a run of equal points across waves and a trip
    "two_points_n12": (two_points, (), 4, 12, 1, (0,), None),
    "line_horizontal": (line, ("horizontal",), 6, 100, 2, (0,), None),            # ties in the exact +-y directions, cnt = n
    "line_vertical": (line, ("vertical",), 7, 100, 3, (0,), None),                # one equal-x run: the sort orders by y alone
    "line_slope_3_7": (line, ("slope",), 9, 100, 4, (0,), None),
    "three_collinear": (three_collinear, (), 2, 3, 1, (0,), None),                # cnt = 3, the hull has 2 vertices
    # equal-x runs and lattice ties: vertical hull edges, 15 collinear points on every edge, edges tying in +-x and +-y
    "grid17": (grid, (17,), 11, 289, 5, (0,), None),                              # 64 survivors: cnt = 64, a power of two
    "grid17_dup_corners": (grid_dup_corners, (17,), 11, 297, 6, (0,), None),      # 72 survivors: INFINITY padding to 128
    "grid65": (grid, (65,), 13, 4225, 7, (0,), None),                             # n > cap, the 256 boundary points survive
    "circle65": (circle, (65,), 10, 13273, 8, (0,), None),
    # duplicate runs across wave, trip, workgroup and pad boundaries
    "dup_boundaries": (dup_boundaries, (), 5, 5000, 9, (1, 3, 0), None),
    # chain sizes: n survivors by construction; 1025 .. 4096 on the device (4096: two trips of the compare-exchange loop), 4097 over
    "parabola_1025": (parabola, (), 3, 1025, 10, (0,), "device"),
    "parabola_2048": (parabola, (), 6, 2048, 11, (0,), "device"),
    "parabola_2049": (parabola, (), 3, 2049, 12, (0,), "device"),
    "parabola_4096": (parabola, (), 3, 4096, 13, (0,), "device"),
    "parabola_4097": (parabola, (), 3, 4097, 14, (0,), "host"),
    "over_cap_vertex": (over_cap_vertex, (), 4, 4300, 15, (0,), "host"),          # 4200 copies of one vertex: the lowest index
    # k_chnmf_proj: every m % 4, one and many k-steps, m across the 64-row pad
    "proj_m2": (proj_figure, (2,), 2, 320, 20, (0,), None),
    "proj_m3": (proj_figure, (3,), 3, 320, 21, (0,), None),
    "proj_m4": (proj_figure, (), 4, 320, 22, (0,), None),
    "proj_m5": (proj_figure, (), 5, 320, 23, (0,), None),
    "proj_m7": (proj_figure, (), 7, 320, 24, (0,), None),
    "proj_m8": (proj_figure, (), 8, 320, 25, (0,), None),
    "proj_m9": (proj_figure, (), 9, 320, 26, (0,), None),
    "proj_m16": (proj_figure, (), 16, 320, 27, (0,), None),
    "proj_m17": (proj_figure, (), 17, 320, 28, (0,), None),
    "proj_m63": (proj_figure, (), 63, 320, 29, (0,), None),
    "proj_m64": (proj_figure, (), 64, 320, 30, (0,), None),
    "proj_m65": (proj_figure, (), 65, 320, 31, (0,), None),
    "proj_m127": (proj_figure, (), 127, 320, 32, (0,), None),
    "proj_m1000": (proj_figure, (), 1000, 100, 33, (0,), None),
    "proj_m4099": (proj_figure, (), 4099, 100, 34, (0,), None),
    # ... and n an exact multiple of 64 and of 256, one past it, and a multiple of 64 that is none of 256
    "proj_n64": (proj_figure, (), 9, 64, 35, (0,), None),
    "proj_n256": (proj_figure, (), 9, 256, 36, (0,), None),
    "proj_n257": (proj_figure, (), 9, 257, 37, (0,), None),
    "proj_n4160": (proj_figure, (), 9, 4160, 38, (0,), None),
    # all 16 rows of R: 120 pairs back to back through the shared scratch buffers
    "rows16_m16": (rows16, (), 16, 1061, 40, (0,), None),
    "rows16_m37": (rows16, (), 37, 1061, 40, (0,), None),
    # 1025 panels, two per workgroup
    "panel_8x65600": (panel_corners, (), 8, 65600, 41, (0,), None),
}
PROJ_M = [2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64, 65, 127, 1000, 4099]
FORCED_CAP = 64                                                    # survivor_cap of the rerun / host runs of ...
FORCED_CAP_CASES = ["grid17_dup_corners", "line_slope_3_7", "grid65"]    # ... 72, 100 and 256 survivors

_cache = {}


def case(name):
    """dict(P int64 targets, V float32, R float64, m, n, base_sel, max_wgs, routes, hull int32): built once, never written to."""
    if name not in _cache:
        fig, args, m, n, seed, max_wgs, routes = CASES[name]
        P = fig(n, seed, *args)
        assert P.shape[1] == n and P.dtype == np.int64, (name, P.shape)
        V, R = build(P, m, 1000 + seed)
        hull = exact_union(P)
        for a in (P, V, R, hull):
            a.setflags(write=False)
        _cache[name] = dict(P=P, V=V, R=R, m=m, n=n, base_sel=P.shape[0], max_wgs=max_wgs, routes=routes, hull=hull)
    return _cache[name]
