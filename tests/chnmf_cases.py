"""The CHNMF fixtures (tests/golden/chnmf_*.npz, made by tests/golden/gen_golden_chnmf.py from the real pymf/chnmf.py) and what
makes the device's answer on them determinate.

The device forms proj = R V in float64 with another summation order than NumPy.  Two float64 summation orders of one entry of
proj differ by at most

    gamma = 2 rows 2^-53 max_{s, c} sum_r |R[s, r]| |V[r, c]|

(each order is within rows 2^-53 sum |terms| of the exact sum).  A fixture is determinate when, in every pair of projected
coordinates, moving every point by gamma cannot change the hull: with TAU = 1e4 gamma

  * every hull vertex lies outside the hull of the remaining points by more than TAU,
  * every other point lies inside the hull by more than TAU,
  * two points that are not bit-identical differ by more than TAU in some coordinate.

Bit-identical points (the `dups` fixture) count as one point, at their lowest index: the reference's vq returns the first
index among duplicates (chnmf.py:167), and identical columns of V give identical projections in any ONE summation order.

chain_hull is a plain NumPy restatement of the device's stage 2 (sort by (x, y, index), monotone chain with a strict turn
test, the first of a run of equal points); filter_survivors restates stage 1 (the extremes in D directions, then everything
inside their polygon by more than the margin is discarded).  Neither is the reference's quickhull: the goldens carry that."""
import itertools
import math

import numpy as np

from conftest import load_golden

FIXTURES = ["chnmf_doc_2x3_k2", "chnmf_29x300_k6_sel3", "chnmf_37x1061_k5_sel5", "chnmf_8x5000_k4_sel2_ring", "chnmf_29x300_dups"]
RING = "chnmf_8x5000_k4_sel2_ring"
DUPS = "chnmf_29x300_dups"
CAP = 4096                # PMF_CH_CAP
D0, D1 = 32, 128          # PMF_CH_D0, PMF_CH_D1

_cache = {}


def fixture(name):
    """The golden as a dict, with base_sel and k as ints; loaded once, never written to."""
    if name not in _cache:
        g = load_golden(name)
        g["k"], g["base_sel"], g["seed"] = int(g["k"]), int(g["base_sel"]), int(g["seed"])
        for v in g.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def proj64(V, R):
    """R V in float64, every entry in the same summation order (identical columns give identical points; a blocked BLAS sums a
    column by its position)."""
    return np.einsum("sr,rc->sc", np.asarray(R, dtype=np.float64), np.asarray(V, dtype=np.float64))


def gamma(V, R):
    V, R = np.asarray(V, dtype=np.float64), np.asarray(R, dtype=np.float64)
    return 2.0 * V.shape[0] * 2.0 ** -53 * np.abs(R).dot(np.abs(V)).max()


def pairs(base_sel):
    return list(itertools.combinations(range(base_sel), 2))


def _cross(ox, oy, ax, ay, bx, by):
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox)


def chain_hull(x, y, idx=None):
    """Stage 2: the sample indices of the strict hull vertices of the points (x[q], y[q]) with sample indices idx[q] (default
    0 .. n - 1), counter-clockwise from the lowest (x, y)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    idx = np.arange(x.shape[0]) if idx is None else np.asarray(idx)
    order = np.lexsort((idx, y, x))
    xs, ys, ids = x[order], y[order], idx[order]
    first = np.ones(xs.shape[0], dtype=bool)
    first[1:] = (xs[1:] != xs[:-1]) | (ys[1:] != ys[:-1])
    out = []
    for side in (0, 1):
        st = []
        rng = range(xs.shape[0]) if side == 0 else range(xs.shape[0] - 1, -1, -1)
        for p in rng:
            if not first[p]:
                continue
            while len(st) >= 2 and _cross(xs[st[-2]], ys[st[-2]], xs[st[-1]], ys[st[-1]], xs[p], ys[p]) <= 0.0:
                st.pop()
            st.append(p)
        out.extend(st[:-1] if len(st) > 1 else st)
    seen, verts = set(), []
    for p in out:
        if p not in seen:
            seen.add(p)
            verts.append(int(ids[p]))
    return verts


def hull_union(V, R):
    """_hull_idx by stage 2 alone, on the float64 projection of NumPy."""
    P = proj64(V, R)
    found = set()
    for i, j in pairs(P.shape[0]):
        found.update(chain_hull(P[i], P[j]))
    return np.array(sorted(found), dtype=np.int32)


def directions(D):
    """The D filter directions: angle 2 pi t / D, with +-x and +-y exact."""
    out = np.zeros((D, 2))
    for t in range(D):
        q, r = divmod(t, D // 4)
        a = 2.0 * math.pi * r / D
        cs, sn = (1.0, 0.0) if r == 0 else (math.cos(a), math.sin(a))
        out[t] = [(cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs)][q]
    return out


def filter_survivors(x, y, D):
    """Stage 1: the ascending indices of the points that are NOT inside every edge of the polygon of the D extremes by more than
    64 2^-53 scale (|ex| + |ey|)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = directions(D)
    ext = np.argmax(d[:, :1] * x[None, :] + d[:, 1:] * y[None, :], axis=1)      # (the first index attaining the maximum)
    scale = max(np.abs(x).max(), np.abs(y).max())
    vx, vy = x[ext], y[ext]
    ex, ey = np.roll(vx, -1) - vx, np.roll(vy, -1) - vy
    live = (ex != 0.0) | (ey != 0.0)
    if not live.any():
        return np.arange(x.shape[0])
    inside = np.ones(x.shape[0], dtype=bool)
    for t in np.nonzero(live)[0]:
        cr = ex[t] * (y - vy[t]) - ey[t] * (x - vx[t])
        inside &= cr > 64.0 * 2.0 ** -53 * scale * (abs(ex[t]) + abs(ey[t]))
    return np.nonzero(~inside)[0]


def _seg_dist(px, py, ax, ay, bx, by):
    """Distance of the point p to the segment a b."""
    dx, dy = bx - ax, by - ay
    L = dx * dx + dy * dy
    t = 0.0 if L == 0.0 else min(1.0, max(0.0, ((px - ax) * dx + (py - ay) * dy) / L))
    return math.hypot(px - (ax + t * dx), py - (ay + t * dy))


def pair_margins(x, y):
    """(vertex margin, interior margin, separation) of one pair's points, bit-identical points taken once:
    the least distance of a hull vertex to the hull of the remaining points, the least distance of a non-vertex to the hull's
    boundary (negative if outside), the least Chebyshev distance between two distinct points."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    pts = np.unique(np.stack([x, y], axis=1), axis=0)           # sorted by (x, y), duplicates merged
    x, y = pts[:, 0], pts[:, 1]
    n = x.shape[0]
    # separation: in the (x, y) order two points closer than s in both coordinates are within s in x
    sep = np.inf
    dx = np.diff(x)
    for q in np.nonzero(dx <= 1e-6 * max(np.abs(x).max(), 1e-300))[0]:
        r = q + 1
        while r < n and x[r] - x[q] <= 1e-6 * np.abs(x).max():
            sep = min(sep, max(x[r] - x[q], abs(y[r] - y[q])))
            r += 1
    sep = min(sep, 1e-6 * np.abs(x).max()) if n > 1 else np.inf
    verts = chain_hull(x, y)
    h = len(verts)
    if h < 3:
        return np.inf, np.inf, sep
    hx, hy = x[verts], y[verts]
    # interior: signed distance to every edge line of the counter-clockwise hull, positive inside
    ex, ey = np.roll(hx, -1) - hx, np.roll(hy, -1) - hy
    el = np.hypot(ex, ey)
    is_vertex = np.zeros(n, dtype=bool)
    is_vertex[verts] = True
    rest = np.nonzero(~is_vertex)[0]
    inner = np.inf
    if rest.size:
        sd = (ex[None, :] * (y[rest, None] - hy[None, :]) - ey[None, :] * (x[rest, None] - hx[None, :])) / el[None, :]
        inner = sd.min()
    # vertices: without v the hull changes between v's neighbours a and b only, by the points inside the triangle a v b
    outer = np.inf
    for q in range(h):
        a, v, b = verts[q - 1], verts[q], verts[(q + 1) % h]
        if h == 3:
            cand = np.nonzero(np.arange(n) != v)[0]
        else:
            c1 = _cross(x[a], y[a], x[v], y[v], x, y)
            c2 = _cross(x[v], y[v], x[b], y[b], x, y)
            c3 = _cross(x[b], y[b], x[a], y[a], x, y)
            cand = np.nonzero((c1 >= 0) & (c2 >= 0) & (c3 >= 0) & (np.arange(n) != v))[0]
            cand = np.union1d(cand, [a, b])
        loc = chain_hull(x[cand], y[cand], cand)
        m = len(loc)
        dist = min(_seg_dist(x[v], y[v], x[loc[s]], y[loc[s]], x[loc[(s + 1) % m]], y[loc[(s + 1) % m]]) for s in range(m)) if m > 1 else \
            math.hypot(x[v] - x[loc[0]], y[v] - y[loc[0]])
        outer = min(outer, dist)
    return outer, inner, sep


def margins(V, R):
    """The least of pair_margins over all pairs, and TAU."""
    P = proj64(V, R)
    worst = [np.inf, np.inf, np.inf]
    for i, j in pairs(P.shape[0]):
        worst = [min(w, m) for w, m in zip(worst, pair_margins(P[i], P[j]))]
    return tuple(worst) + (1e4 * gamma(V, R),)


def determinate(V, R):
    outer, inner, sep, tau = margins(V, R)
    return outer > tau and inner > tau and sep > tau
