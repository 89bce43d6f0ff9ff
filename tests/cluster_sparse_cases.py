"""The device cases of Kmeans and Cmeans on scipy.sparse data (tests/test_gpu_cluster_sparse.py) and what makes the comparison with
the float64 oracle on toarray() meaningful (tests/test_cluster_sparse_cases.py, no GPU): the smallest shapes at which
k_cluster_csr_assign, k_cluster_csr_num and k_cluster_csr_finish can go wrong.

Data: planted sparse clusters.  Centres (0.25 + rand(m, nb)) on a random support of fraction s; a sample is the centre of its
label + 0.05 randn on that support, masked by Bernoulli(0.5).  Then, as in tests/cur_sparse_cases.py, row m // 3 and column n // 3
are filled completely (the long lines: the filled row has n - 2 entries and is cut into chunks by the W step) and after that rows
m // 2 and m - 1 and columns n // 2 and 0 are emptied (a zero sample is at distance |w_c| from every centre).  float32.
W0 = 0.5 centres + 0.02 randn on the support.  Cmeans starts from W0 and H0 = RandomState(7).random_sample((k, n)).

The yardstick is tests/cluster_oracle.py in float64 on toarray().  The seed of a case is the first one from 1 on whose 3-iteration
Kmeans run keeps every assignment gap (d2 - d1) / |v| >= MIN_GAP, the figure of tests/test_gpu_cluster.py, with at least two members in
every centre after every H step (tests/test_cluster_sparse_cases.py asserts both).  The wide case has a gap of about 1e-5: Kmeans is
checked there sample by sample against the oracle's distances, one H step only.

ferr on sparse data: Kmeans right behind its own H step sqrt(sum min d^2), otherwise the identity
ferr^2 = ||data||^2 - 2 <W^T data, H> + <W^T W, H H^T>, both in float64.  The identity's deviation from the direct norm on the
oracle's factors, relative to ||data||, is what its cancellation is worth on these data; the device is held to FACTOR x the worst of
them, floored at cur_sparse_cases.FERR_FLOOR (tests/golden/cluster_sparse_tolerances.json), against the direct float64 norm
(cluster_oracle.frobenius) on toarray() and the factors that the device returned: W is rounded to float32 by every W step, so the
oracle's own trajectory, which keeps W in float64, differs from the device's in first order of 6e-8 (Kmeans too: its W is the
minimiser of the error for the assignment it was formed from, not for the next one), and is compared at the 2e-5 of DESIGN.md
section 4 like W and H.
"""
import json
import math
import os

import numpy as np
import scipy.sparse as sp

import cluster_oracle as co
from cnmf_oracle import _converged
from cur_cases import FACTOR

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "golden", "cluster_sparse_tolerances.json")

# constants of the headers that decide which branch a case reaches (tests/test_cluster_sparse_cases.py reads them back)
WAVE = 64                # entries a wave loads at a time
MIN_LINES = 64           # PMF_CCSR_MIN_LINES: samples per workgroup of the H step at least
MAX_WGS = 1024           # PMF_CL_MAX_WGS: partials
CHUNK = 512              # PMF_CCSR_CHUNK: entries of a data row per wave of the W step
MIN_GAP = 1e-4
NITER = 3

# name: (rows, cols, num_bases, support fraction, seed)
SPARSE_CASES = {
    "29x300_k5": (29, 300, 5, 0.4, 1),           # every sample shorter than one load; k under 16
    "151x700_k8": (151, 700, 8, 0.2, 1),         # the filled sample has 149 = 2 * 64 + 21 entries: a tail of one; 11 workgroups, the last ragged
    "300x5000_k64": (300, 5000, 64, 0.1, 1),     # a full half of centres; the filled row: 10 chunks, the last with 390 entries
    "1100x700_k6": (1100, 700, 6, 0.05, 1),      # tall
    "80x4500_k33": (80, 4500, 33, 0.3, 1),       # k not a multiple of 16, past 32
    "2100x4100_k128": (2100, 4100, 128, 0.04, 1),  # two halves of centres; the filled row: 9 chunks, the last with 2 entries
}
WIDE_CASE = "48x66000_k3"
WIDE = (48, 66000, 3, 0.3, 1)                    # more than 64 * 1024 samples: 68 per workgroup, 971 workgroups, the last ragged


def shape(name):
    return WIDE if name == WIDE_CASE else SPARSE_CASES[name]


def planted(m, n, nb, s, seed):
    """(canonical float32 csr_matrix, W0 float64, labels)."""
    rs = np.random.RandomState(seed)
    C = 0.25 + rs.rand(m, nb)
    S = rs.rand(m, nb) < s
    labels = rs.randint(0, nb, size=n)
    d = (C[:, labels] + 0.05 * rs.randn(m, n)) * S[:, labels] * (rs.rand(m, n) < 0.5)
    d[m // 3, :] = 0.25 + rs.rand(n)
    d[:, n // 3] = 0.25 + rs.rand(m)
    for r in (m // 2, m - 1):
        d[r, :] = 0.0
    for c in (n // 2, 0):
        d[:, c] = 0.0
    W0 = (0.5 * C + 0.02 * rs.randn(m, nb)) * S
    A = sp.csr_matrix(d.astype(np.float32))
    A.eliminate_zeros()
    A.sum_duplicates()
    return A, W0, labels


def kmeans_run(d64, W0, niter):
    """cluster_oracle.kmeans from W0, also keeping the gap and the smallest member count of every H step."""
    k = W0.shape[1]
    W = np.array(W0)
    assigned, H, g = co.kmeans_update_h(d64, W)
    gaps, members = [g], [int(np.bincount(assigned, minlength=k).min())]
    ferr = np.zeros(niter)
    for i in range(niter):                                            # nmf.py:182-202
        W = co.kmeans_update_w(d64, W, assigned)
        assigned, H, g = co.kmeans_update_h(d64, W)
        gaps.append(g)
        members.append(int(np.bincount(assigned, minlength=k).min()))
        ferr[i] = co.frobenius(d64, W, H)
        if i > 1 and _converged(ferr, i, d64.shape[1]):
            ferr = ferr[:i]
            break
    return dict(W=W, H=H, assigned=assigned, ferr=ferr, gaps=gaps, members=members)


def identity_ferr(d64, W, H):
    """The trace identity of the module docstring in float64, ||data||^2 as the sum of the row norms."""
    vn = float(np.sum(np.sum(d64 ** 2, axis=1)))
    f2 = vn - 2.0 * float(np.sum(np.dot(W.T, d64) * H)) + float(np.sum(np.dot(W.T, W) * np.dot(H, H.T)))
    return float(np.sqrt(max(f2, 0.0)))


_cache = {}


def case(name):
    """dict(sparse csr float32, data dense float32, d64, num_bases, W0, H0, norm, kmeans=kmeans_run(...), cmeans=dict(W, H, ferr)):
    the float64 oracle of Kmeans / Cmeans .factorize(niter=3) on toarray().  The wide case holds one H step each instead:
    kmeans=dict(dist [k][n], assigned, H), cmeans=dict(H)."""
    if name not in _cache:
        m, n, k, s, seed = shape(name)
        A, W0, _ = planted(m, n, k, s, seed)
        d = A.toarray()
        d64 = d.astype(np.float64)
        H0 = np.random.RandomState(7).random_sample((k, n))
        c = dict(sparse=A, data=d, d64=d64, num_bases=k, W0=W0, H0=H0, norm=float(np.linalg.norm(d64)))
        if name == WIDE_CASE:
            W32 = W0.astype(np.float32).astype(np.float64)             # the W that the device holds
            assigned, H, gap = co.kmeans_update_h(d64, W32)
            c["W32"] = W32
            c["kmeans"] = dict(dist=co.pdist(W32, d64), assigned=assigned, H=H, gap=gap)
            c["cmeans"] = dict(H=co.cmeans_update_h(d64, W32))
        else:
            c["kmeans"] = kmeans_run(d64, W0, NITER)
            Wc, Hc, fc = co.cmeans(d64, W0, H0, niter=NITER)
            c["cmeans"] = dict(W=Wc, H=Hc, ferr=fc)
        _cache[name] = c
    return _cache[name]


def find_seed(m, n, k, s, first=1, last=20):
    """The first seed whose Kmeans run keeps MIN_GAP and two members per centre."""
    for seed in range(first, last + 1):
        A, W0, _ = planted(m, n, k, s, seed)
        r = kmeans_run(A.toarray().astype(np.float64), W0, NITER)
        if min(r["gaps"]) >= MIN_GAP and min(r["members"]) >= 2:
            return seed
    return None


def round_up_2(x):
    """x rounded up to two significant digits."""
    if x <= 0.0:
        return 0.0
    e = int(math.floor(math.log10(x))) - 1
    return float("%.1e" % (math.ceil(x / 10.0 ** e * (1.0 - 1e-12)) * 10.0 ** e))


def measure():
    """Per case: the deviation of the identity from the direct error on the oracle's factors, relative to ||data||, for the Kmeans
    and the Cmeans factors, and ferr / ||data||."""
    out = {}
    for name in SPARSE_CASES:
        c = case(name)
        row = {}
        for kind in ("kmeans", "cmeans"):
            W, H = c[kind]["W"], c[kind]["H"]
            direct = co.frobenius(c["d64"], W, H)
            row[kind] = abs(identity_ferr(c["d64"], W, H) - direct) / c["norm"]
            row[kind + "_rel"] = direct / c["norm"]
        out[name] = row
    return out


def tolerances():
    """The committed figures (tests/golden/cluster_sparse_tolerances.json, written by tests/golden/gen_golden_cluster_sparse.py)."""
    with open(TOL_PATH) as f:
        return json.load(f)


def device_tol_ferr():
    """FACTOR x the largest committed identity-vs-direct deviation over all cases, floored at cur_sparse_cases.FERR_FLOOR."""
    import cur_sparse_cases as csc
    return max(FACTOR * tolerances()["ferr_max"], csc.FERR_FLOOR)


# ---- which branch a case reaches, from the constants above ---------------------------------------------------------------------
def lines_per_wg(n):
    return -(-max(MIN_LINES, -(-n // MAX_WGS)) // 4) * 4


def workgroups(n):
    return -(-n // lines_per_wg(n))


def chunks(A):
    """Chunks per data row of the W step."""
    return -(-np.diff(A.indptr) // CHUNK)
