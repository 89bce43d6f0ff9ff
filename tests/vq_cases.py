"""Cases for vq / pdist (pymf_amd.distance, pmf_vq_columns / pmf_vq_assign): tests/test_vq_cases.py checks them without a GPU,
tests/test_gpu_vq.py runs them on the device.

EXACT cases: data V (m x n) and queries Q (m x nq) hold integers with |value| <= 64 and m <= 65, so every difference
(<= 128), every square (<= 2^14) and every partial sum (<= 65 * 2^14 < 2^24) is an integer that float32 represents: the l1
distance and the squared l2 distance come out exactly in any summation order, and float32's square root, monotone, keeps ties
ties and -- below 2^21 two distinct integers have roots more than two units in the last place apart -- distinct sums distinct.
The expected answers are integer arithmetic (int64: D1 = sum |v - q|, D2 = sum (v - q)^2, np.argmin = the lowest index among
equal ones); every exact case is held with array_equal alone.
Planted ties (tie_plan): for a pair of columns (a, b) on both sides of a boundary of the sweep -- a lane's quad (4 columns), a
64-column panel = a workgroup's range while n <= 65 536, a wave (256 columns) and a trip of the workgroup (1024 columns) inside
the wider ranges of the deep cases, the last column before the pad -- one query q with Q[0, q] = an anchor (62, 58, ... 46) and
V[:, a] = q + e0, V[:, b] = q - e0: two DIFFERENT columns at distance 1 from it, everything else (first coordinate in
[-30, 30], or around another anchor) at least 3 away; the lower column must win.  The same for the assign direction: a column
c with V[0, c] = an anchor (-62, -58, ... -34) and two queries c - e0, c + e0 at (j1, j2) on both sides of a tile of 16
queries (or the first and the last query).  One more query is the zero
vector while no data column is: the zero PAD columns of the device image are nearer to it than any real column and must
never be offered.

GENERIC cases: random float32 data (one set offset by 1e3 from the origin), m up to 300 and one of 1100 rows (more than one
slab of 512 rows in LDS), expected = ref_pdist: the reference's
float64 arithmetic (dist.py:33, dist.py:61) on the float32-rounded inputs.  EPS(m) = (m + 4) 2^-24: each term carries at most
3 roundings (difference, square, its addition), the sum of m non-negative terms m - 1 more, the root one.  A returned
distance must be within EPS d_ref; where the relative gap between the nearest and the second nearest reference distance
exceeds 2 EPS the index must be the reference's, otherwise its reference distance must be within (1 + 2 EPS) of the smallest.
generic_case asserts that at least 95 % of the decisions of every case lie above the gap.

Nothing here imports the library or needs a GPU."""
import numpy as np

TILE = 16                 # PMF_VQ_TILE
MAX_Q = 128               # PMF_VQ_MAX_Q
MAX_WGS = 1024            # PMF_CL_MAX_WGS
LDS_FLOATS = 8192         # PMF_VQ_LDS
METRICS = ("l2", "l1")
BOUND = 64


def eps(m):
    return (m + 4) * 2.0 ** -24


# ---- the sweep's geometry (pmf_host_cluster.h: panel_partition)
def partition(n):
    """(columns a workgroup owns, workgroups) of a sweep over n columns."""
    npanels = (n + 63) // 64
    want = min(npanels, MAX_WGS)
    ppw = (npanels + want - 1) // want
    return 64 * ppw, (npanels + ppw - 1) // ppw


# ---- exact integer distances
def int_dists(V, Q):
    """(D1, D2) [nq][n] int64: sum |v - q| and sum (v - q)^2, row by row (no m x nq x n intermediate)."""
    V, Q = np.asarray(V, dtype=np.int64), np.asarray(Q, dtype=np.int64)
    D1 = np.zeros((Q.shape[1], V.shape[1]), dtype=np.int64)
    D2 = np.zeros_like(D1)
    for r in range(V.shape[0]):
        d = V[r][None, :] - Q[r][:, None]
        D1 += np.abs(d)
        D2 += d * d
    return D1, D2


class ExactCase(object):
    def __init__(self, name, V, Q, col_ties, asg_ties):
        self.name, self.col_ties, self.asg_ties = name, col_ties, asg_ties
        assert V.dtype == np.int64 and Q.dtype == np.int64 and V.shape[0] == Q.shape[0]
        self.m, self.n = V.shape
        self.nq = Q.shape[1]
        assert self.m <= 65 and 1 <= self.nq <= MAX_Q
        assert int(np.abs(V).max()) <= BOUND and int(np.abs(Q).max()) <= BOUND
        self.Vi, self.Qi = V, Q
        self.V, self.Q = V.astype(np.float32), Q.astype(np.float32)
        self.D1, self.D2 = int_dists(V, Q)
        assert int(self.D2.max()) < 2 ** 21 and int(self.D1.max()) < 2 ** 24      # exact in float32, distinct roots distinct
        self.D = {"l1": self.D1, "l2": self.D2}
        # vq in both directions: per query the nearest column, per column the nearest query; lowest index on ties
        self.cols = {k: np.argmin(d, axis=1) for k, d in self.D.items()}
        self.asg = {k: np.argmin(d, axis=0) for k, d in self.D.items()}

    def squared(self, metric, d):
        """d [nq][n] float64 as returned, as the integers to compare with D[metric] by array_equal: l1 itself; l2: the float32
        root widened, whose square rounds back to the exact integer (relative error 2^-23 of at most 2^21: below 1/2)."""
        d = np.asarray(d)
        assert d.dtype == np.float64 and d.shape == self.D1.shape
        return d if metric == "l1" else np.rint(d * d)

    def rounded_root(self):
        """The correctly rounded float32 root of D2, widened: what an IEEE sqrtf returns for l2 (reported, not asserted)."""
        return np.sqrt(self.D2.astype(np.float32)).astype(np.float64)


def tie_plan(n, nq):
    """The column pairs (a, b) and the (column, query, query) triples whose boundaries exist at this shape."""
    wg_cols, wgs = partition(n)
    pairs = []
    edges = [e for e in (256, 1024) if e < wg_cols] + [wg_cols, wg_cols * (wgs - 1), n - 1, 4, 64]   # (the widest ranges first)
    for edge in edges:
        if 0 < edge < n and (edge - 1, edge) not in pairs:
            pairs.append((edge - 1, edge))
    free = []
    for c in (0, 2, 5, 62, 66, 254, 258, 1022, 1026, wg_cols - 2, wg_cols + 1, n - 3):
        if 0 <= c < n and c not in free and all(c not in p for p in pairs):
            free.append(c)
    qpairs = [(0, nq - 1)] if nq >= 2 else []
    for edge in range(TILE, nq, TILE):
        qpairs.append((edge - 1, edge))
    return pairs, free, qpairs[:8]


def exact_case(m, n, nq, seed):
    rng = np.random.RandomState(seed)
    V = rng.randint(-30, 31, size=(m, n)).astype(np.int64)
    Q = rng.randint(-30, 31, size=(m, nq)).astype(np.int64)
    V[0, V[0] == 0] = 1                                  # no zero column: the zero query's nearest is a real one
    pairs, free, qpairs = tie_plan(n, nq)
    used = set()
    asg_ties = []
    for (j1, j2), c in zip(qpairs, free):
        if j1 == j2 or j1 in used or j2 in used:
            continue
        anchor = -62 + 4 * len(asg_ties)                 # (an anchor of its own per tie: with one row the ties must not meet)
        V[0, c] = anchor
        Q[:, j1] = V[:, c]; Q[0, j1] = anchor - 1
        Q[:, j2] = V[:, c]; Q[0, j2] = anchor + 1
        used.update((j1, j2))
        asg_ties.append((c, j1, j2))
    spare = [j for j in range(nq) if j not in used]
    col_ties = []
    zero_q = None
    if len(spare) > len(pairs[:1]):                      # (the ties come first: a single query goes to a tie)
        zero_q = spare.pop()
        Q[:, zero_q] = 0
    for (a, b), j in zip(pairs[:5], spare):
        anchor = 62 - 4 * len(col_ties)
        Q[0, j] = anchor
        V[:, a] = Q[:, j]; V[0, a] = anchor + 1
        V[:, b] = Q[:, j]; V[0, b] = anchor - 1
        col_ties.append((a, b, j))
    case = ExactCase("m%d_n%d_q%d" % (m, n, nq), V, Q, col_ties, asg_ties)
    case.zero_q = zero_q
    # the builder's own invariants: every planted tie is the minimum, attained exactly twice, and the lower index is expected
    for a, b, j in col_ties:
        for k, d in case.D.items():
            assert d[j, a] == d[j, b] == 1 and int((d[j] == 1).sum()) == 2 and int(d[j].min()) == 1, (case.name, k, a, b, j)
            assert case.cols[k][j] == a
    for c, j1, j2 in asg_ties:
        for k, d in case.D.items():
            assert d[j1, c] == d[j2, c] == 1 and int((d[:, c] == 1).sum()) == 2 and int(d[:, c].min()) == 1, (case.name, k, c, j1, j2)
            assert case.asg[k][c] == j1
    if zero_q is not None:
        assert int(case.D1[zero_q].min()) > 0            # the pad columns (distance 0) would beat every real column
    return case


M_SET = (1, 3, 4, 5, 7, 64, 65)
N_SET = (1, 63, 64, 65, 257)
Q_SET = (1, 15, 16, 17, 64, 65, 128)
# beyond 65 536 columns a workgroup owns more than one panel: one column past 1024 one-panel ranges (two panels each, 513
# workgroups), past 1024 four-panel ranges (five panels: a wave boundary inside the range) and past 1024 sixteen-panel ranges
# (17 panels = 1088 columns: a second trip of the workgroup, 64 of its 256 lanes live)
DEEP = ((3, 64 * MAX_WGS + 1, 17), (4, 4 * 64 * MAX_WGS + 1, 8), (1, 16 * 64 * MAX_WGS + 1, 8))


def exact_shapes():
    """Every (m, n, nq) of the three sets, and the deep shapes."""
    return [(m, n, q) for m in M_SET for n in N_SET for q in Q_SET] + list(DEEP)


def exact_seed(m, n, nq):
    return 1000003 * m + 101 * n + nq


_EXACT = {}


def exact(m, n, nq):
    key = (m, n, nq)
    if key not in _EXACT:
        _EXACT[key] = exact_case(m, n, nq, exact_seed(m, n, nq))
    return _EXACT[key]


# ---- generic cases
def ref_pdist(Q, V, metric):
    """The float64 distance block [nq][n] of the float32 inputs, one query at a time from the difference, summed down the rows --
    the arithmetic of the reference's pdist(Q, V) for nq <= n (tests/test_vq_cases.py holds it to the recorded goldens bit for bit)."""
    Q, V = np.asarray(Q, dtype=np.float64), np.asarray(V, dtype=np.float64)
    out = np.empty((Q.shape[1], V.shape[1]))
    for j in range(Q.shape[1]):
        delta = V - Q[:, [j]]
        out[j] = np.sqrt(np.square(delta).sum(axis=0)) if metric == "l2" else np.abs(delta).sum(axis=0)
    return out


class GenericCase(object):
    def __init__(self, name, V, Q):
        self.name = name
        self.V, self.Q = np.ascontiguousarray(V, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)
        self.m, self.n = self.V.shape
        self.nq = self.Q.shape[1]
        self.eps = eps(self.m)
        self.ref = {k: ref_pdist(self.Q, self.V, k) for k in METRICS}
        self.above = {}
        for k, d in self.ref.items():
            for axis, tag in ((1, "cols"), (0, "asg")):
                if d.shape[axis] < 2:
                    self.above[k, tag] = np.ones(d.shape[1 - axis], dtype=bool)
                    continue
                two = np.partition(d, 1, axis=axis)
                lo, hi = np.take(two, 0, axis=axis), np.take(two, 1, axis=axis)
                self.above[k, tag] = (hi - lo) > 2.0 * self.eps * lo
            assert all(self.above[k, t].mean() >= 0.95 for t in ("cols", "asg")), (name, k)

    def check_dist(self, metric, d):
        """largest |d - d_ref| / (EPS d_ref) over the block (must be <= 1)."""
        ref = self.ref[metric]
        return float((np.abs(np.asarray(d) - ref) / (self.eps * np.maximum(ref, np.finfo(np.float64).tiny))).max())

    def check_index(self, metric, tag, idx):
        """True when every index is the reference's above the gap and within (1 + 2 EPS) of the smallest below it."""
        ref = self.ref[metric] if tag == "cols" else self.ref[metric].T          # [decision][candidate]
        idx = np.asarray(idx)
        want = np.argmin(ref, axis=1)
        above = self.above[metric, tag]
        got = ref[np.arange(ref.shape[0]), idx]
        return bool(np.array_equal(idx[above], want[above]) and (got <= (1.0 + 2.0 * self.eps) * ref.min(axis=1)).all())


def generic_specs():
    """name -> (m, n, nq, seed, offset, kind)"""
    return {
        "uniform_37x1000_q5": (37, 1000, 5, 11, 0.0, "uniform"),
        "uniform_64x4100_q128": (64, 4100, 128, 12, 0.0, "uniform"),
        "offset1e3_29x2049_q33": (29, 2049, 33, 13, 1e3, "uniform"),
        "slabs_300x517_q128": (300, 517, 128, 14, 0.0, "uniform"),          # m QP > 8192 floats: one tile at a time in LDS
        "slabs_65x300_q128": (65, 300, 128, 17, 0.0, "uniform"),            # one row past the whole-image form
        "slabs_1100x300_q17": (1100, 300, 17, 18, 0.0, "uniform"),          # three slabs of 512 rows, restaged per trip and tile
        "centres_16x3000_q9": (16, 3000, 9, 15, 0.0, "centres"),            # samples around 9 centres, the centres as queries
        "normal_7x70000_q17": (7, 70000, 17, 16, 0.0, "normal"),            # two panels per workgroup
    }


def generic_case(name):
    m, n, nq, seed, offset, kind = generic_specs()[name]
    rng = np.random.RandomState(seed)
    if kind == "centres":
        Q = rng.random_sample((m, nq)) * 4.0
        V = Q[:, rng.randint(0, nq, size=n)] + 0.3 * rng.standard_normal((m, n))
    elif kind == "normal":
        V, Q = rng.standard_normal((m, n)), rng.standard_normal((m, nq))
    else:
        V, Q = rng.random_sample((m, n)), rng.random_sample((m, nq))
    return GenericCase(name, V + offset, Q + offset)


_GENERIC = {}


def generic(name):
    if name not in _GENERIC:
        _GENERIC[name] = generic_case(name)
    return _GENERIC[name]
