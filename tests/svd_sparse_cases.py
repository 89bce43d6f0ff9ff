"""The device cases of SVD and PCA on scipy.sparse data (tests/test_gpu_svd_sparse.py) and what makes the comparison with the
float64 oracle (tests/svd_oracle.py on toarray(), cut at k) meaningful (tests/test_svd_sparse_cases.py, no GPU).

Data: a row- and column-permuted direct sum of rank-one blocks s_i u_i v_i^T on disjoint supports, rounded to float32, so the
matrix is sparse (density about 1 / blocks) and its singular values are the blocks' norms: a geometric spectrum.  The step is 1.08
(1.10 where the rank is below 30), except in the two cases that keep 64 and 65 triples: 65 values a step of 1.08 apart span
1.08^128 = 1.9e4 in the eigenvalues, beyond the 1e-4 that the kept eigenvalues must stay within, so those two cases take 1.074
(range 9.3e3; adjacent values still more than 5 % apart).  The k-truncated cases add a sparse random perturbation -- in
130x2100_k64 with one fully dense row (2 100 entries: longer than GRAM_CAP = 256 and than four 64-entry loads) and one fully
dense column -- whose spectral norm is below 1 % of the smallest gap among the kept values (the gap to the first dropped value
included) and below half the smallest kept value.

Tolerances: the deviation of a NumPy twin from the oracle, per quantity, times FACTOR = 4.  The twin does
what the device does: the Gram matrix of the float32 data summed exactly and rounded once to float64 (k_csr_gram adds in exact
fixed point; here: extended precision), eigh, the cut, the projection in float64 with the eigenvectors scaled first.  The oracle
forms the Gram matrix with float64 sums, so the deviation carries the sensitivity of the eigenvectors to one rounding of the Gram
matrix -- what a second eigensolver (Jacobi against LAPACK) is entitled to.  The error is compared as ferr^2 / ||data||^2 (the
identity ||data||^2 - 2 <W^T data, H> + <W^T W, H H^T> against the direct residual): it cancels for an exact fit.  Floors: 1e-13
for vectors, 64 * 2^-52 for ferr^2 / ||data||^2.
"""
import json
import os

import numpy as np

import svd_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "golden", "svd_sparse_tolerances.json")

FACTOR = 4.0
VECTOR_FLOOR = 1e-13
FERR2_FLOOR = 64.0 * 2.0 ** -52
GRAM_CAP = 256            # pmf_csr.h
GRAM_LDS_MAX_NP = 128     # the LDS image of k_csr_gram fits up to this padded width
PROJ_LINES = 16           # PMF_PROJ_LINES (pmf_svd_csr.h): lines a workgroup of k_csr_proj_f64 takes

# name: rows, cols, blocks, seed, largest singular value, step, k, empty (rows and columns outside every block), perturbation density
# (0: none), full (a fully dense row and column in the perturbation)
SVD_CASES = {
    "37x29": dict(rows=37, cols=29, blocks=29, seed=61, smax=8.0, step=1.10, k=-1),                      # tall; odd short side; LDS Gram image
    "29x300": dict(rows=29, cols=300, blocks=29, seed=62, smax=12.0, step=1.10, k=-1),                   # wide; Gram on the transposed image
    "300x40_rank25": dict(rows=300, cols=40, blocks=25, seed=63, smax=12.0, step=1.10, k=-1, empty=2),   # dropped eigenvalues; empty lines
    "2100x130_k65": dict(rows=2100, cols=130, blocks=100, seed=64, smax=30.0, step=1.074, k=65, pert=0.01),   # global Gram slabs; two panels
    "130x2100_k64": dict(rows=130, cols=2100, blocks=100, seed=65, smax=30.0, step=1.074, k=64, pert=0.01, full=True),   # one full panel
    "300x40_k1": dict(rows=300, cols=40, blocks=40, seed=66, smax=12.0, step=1.08, k=1, pert=0.02),      # one kept triple
}
FORMATS_CASE = "37x29"     # also given as csc_matrix and as coo_matrix with duplicate entries
SAME_K_CASE = "37x29"      # k >= short - 1 and k = -1 give the same result

# name: the SVD case whose data it takes, num_bases, a user W with compute_w=False
PCA_CASES = {
    "29x300_nb5": dict(data="29x300", num_bases=5),
    "300x40_nb0": dict(data="300x40_rank25", num_bases=0),
    "29x300_userw": dict(data="29x300", num_bases=4, user_w=True),
}

QUANTITIES = ("U", "V", "S", "ferr2", "orth_proj", "W", "H", "eigenvalues", "pca_ferr2")

_cache = {}


def _groups(rng, extent, blocks, empty):
    """`blocks` disjoint non-empty index groups of a permutation of range(extent), `empty` indices left out."""
    perm = rng.permutation(extent)
    return [g for g in np.array_split(perm[:extent - empty], blocks)]


def dense_data(name):
    """The float32 data of a case as a dense array."""
    if ("dense", name) in _cache:
        return _cache[("dense", name)]
    c = SVD_CASES[name]
    rng = np.random.RandomState(c["seed"])
    rows, cols, blocks = c["rows"], c["cols"], c["blocks"]
    A = np.zeros((rows, cols))
    s = c["smax"] / c["step"] ** np.arange(blocks)
    rg, cg = _groups(rng, rows, blocks, c.get("empty", 0)), _groups(rng, cols, blocks, c.get("empty", 0))
    for i in range(blocks):
        u = rng.uniform(0.5, 1.0, len(rg[i])) * rng.choice([-1.0, 1.0], len(rg[i]))
        v = rng.uniform(0.5, 1.0, len(cg[i])) * rng.choice([-1.0, 1.0], len(cg[i]))
        A[np.ix_(rg[i], cg[i])] = s[i] * np.outer(u / np.linalg.norm(u), v / np.linalg.norm(v))
    if c.get("pert", 0):
        k = c["k"]
        gaps = s[:k] - s[1:k + 1]
        target = 0.5 * min(0.01 * gaps.min(), 0.5 * s[k - 1])   # half of what is allowed: rounding to float32 moves it a little
        E = rng.standard_normal((rows, cols)) * (rng.uniform(size=(rows, cols)) < c["pert"])
        if c.get("full"):
            E[rng.randint(rows), :] = rng.uniform(0.5, 1.0, cols)
            E[:, rng.randint(cols)] = rng.uniform(0.5, 1.0, rows)
        A = A + E * (target / np.linalg.norm(E, 2))
    _cache[("dense", name)] = A.astype(np.float32)
    return _cache[("dense", name)]


def sparse_data(name, fmt="csr"):
    """The data as a scipy.sparse matrix of float32.  fmt "coo_dup": a coo_matrix in which every stored entry v of the first ten
    rows comes as the two entries v / 2 + v / 2 (exact in float32), in reversed order."""
    import scipy.sparse as sp
    A = dense_data(name)
    if fmt == "csr":
        return sp.csr_matrix(A)
    if fmt == "csc":
        return sp.csc_matrix(A)
    coo = sp.coo_matrix(A)
    dup = coo.row < 10
    row = np.concatenate([coo.row[::-1], coo.row[dup]])
    col = np.concatenate([coo.col[::-1], coo.col[dup]])
    half = np.where(dup[::-1], coo.data[::-1] * np.float32(0.5), coo.data[::-1])
    val = np.concatenate([half, coo.data[dup] * np.float32(0.5)]).astype(np.float32)
    return sp.coo_matrix((val, (row, col)), shape=A.shape)


def cut(U, S, V, k, short):
    """The reference's sparse branch (svd.py:165,204): the leading k triples for 0 < k < short - 1, else all."""
    if 0 < k < short - 1:
        return U[:, :k], S[:k, :k], V[:k]
    return U, S, V


def exact_gram(data, left):
    """The Gram matrix of the short side of float32 data: summed in extended precision, rounded once to float64."""
    d = np.asarray(data, dtype=np.longdouble)
    return np.asarray(np.dot(d.T, d) if left else np.dot(d, d.T), dtype=np.float64)


def twin_svd(data, k):
    """(U, S, V) as the device forms them (module docstring)."""
    d64 = np.asarray(data, dtype=np.float64)
    left = d64.shape[0] > d64.shape[1]
    values, vectors = np.linalg.eigh(exact_gram(data, left))
    keep = values > so.EPS
    vectors, values = vectors[:, keep], values[keep]
    idx = np.argsort(values)[::-1]
    if 0 < k < min(d64.shape) - 1:
        idx = idx[:k]
    vectors, s = vectors[:, idx], np.sqrt(values[idx])
    if left:
        return np.dot(d64, vectors / s), np.diag(s), vectors.T
    return vectors, np.diag(s), np.dot(d64.T, vectors / s).T


def ferr2_identity(data, W, H):
    """||data||^2 - 2 <W^T data, H> + <W^T W, H H^T>, clamped at 0, over ||data||^2."""
    d = np.asarray(data, dtype=np.float64)
    n2 = float(np.sum(d * d))
    f2 = n2 - 2.0 * float(np.sum(np.dot(W.T, d) * H)) + float(np.sum(np.dot(W.T, W) * np.dot(H, H.T)))
    return max(f2, 0.0) / n2


def ferr2_direct(data, W, H):
    d = np.asarray(data, dtype=np.float64)
    return float(np.sum((d - np.dot(W, H)) ** 2)) / float(np.sum(d * d))


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.asarray(a).size else 0.0


def orth(P, axis):
    """max |P^T P - I| of the vectors of P (axis 0: columns, 1: rows)."""
    P = np.asarray(P, dtype=np.float64)
    G = np.dot(P.T, P) if axis == 0 else np.dot(P, P.T)
    return float(np.max(np.abs(G - np.eye(G.shape[0]))))


def svd_case(name):
    """dict(data float32 dense, k, left, U, S, V, ferr2): the float64 oracle on toarray(), cut at k."""
    if ("svd", name) not in _cache:
        data, k = dense_data(name), SVD_CASES[name]["k"]
        U, S, V = cut(*so.svd(data.astype(np.float64)), k=k, short=min(data.shape))
        _cache[("svd", name)] = dict(data=data, k=k, left=data.shape[0] > data.shape[1], U=U, S=S, V=V,
                                     ferr2=ferr2_direct(data, U, np.dot(S, V)))
    return _cache[("svd", name)]


def user_w(rows, nb, seed=71):
    return np.linalg.qr(np.random.RandomState(seed).randn(rows, nb))[0]


def pca_case(name):
    """dict(data float32 dense, num_bases, user_w or None, oracle dict(W, H, eigenvalues, ferr2))."""
    if ("pca", name) not in _cache:
        c = PCA_CASES[name]
        data = dense_data(c["data"])
        d64 = data.astype(np.float64)
        if c.get("user_w"):
            W = user_w(data.shape[0], c["num_bases"])
            ora = dict(W=W, H=np.dot(W.T, d64), eigenvalues=None)
        else:
            o = so.pca(d64, c["num_bases"], center_mean=False)
            ora = dict(W=o["W"], H=o["H"], eigenvalues=o["eigenvalues"])
        ora["ferr2"] = ferr2_direct(data, ora["W"], ora["H"])
        ora["data"] = d64
        _cache[("pca", name)] = dict(data=data, num_bases=c["num_bases"], user_w=ora["W"] if c.get("user_w") else None, oracle=ora)
    return _cache[("pca", name)]


def svd_deviation(case, got):
    """Deviation of the (U, S, V) triple `got` from the oracle of `case`, signs fixed on the eigenvector side."""
    left = case["left"]
    Ug, Vg = so.fix_svd_signs(got[0], got[2], left)
    Uw, Vw = so.fix_svd_signs(case["U"], case["V"], left)
    sg, sw = np.diag(got[1]), np.diag(case["S"])
    return dict(U=max_abs(Ug, Uw), V=max_abs(Vg, Vw), S=float(np.max(np.abs(sg - sw) / sw)),
                ferr2=abs(ferr2_identity(case["data"], got[0], np.dot(got[1], got[2])) - case["ferr2"]),
                orth_proj=orth(got[0], 0) if left else orth(got[2], 1))


def pca_deviation(case, got):
    """Deviation of dict(W, H, eigenvalues, ferr2) from the oracle of the PCA case, signs fixed on the eigenvector side."""
    ora = case["oracle"]
    left = case["data"].shape[0] > case["data"].shape[1]
    if case["user_w"] is None:
        from svd_cases import fix_pca_signs
        Wg, Hg = fix_pca_signs(got["W"], got["H"], left)
        Ww, Hw = fix_pca_signs(ora["W"], ora["H"], left)
    else:
        Wg, Hg, Ww, Hw = got["W"], got["H"], ora["W"], ora["H"]
    d = dict(W=max_abs(Wg, Ww), H=max_abs(Hg, Hw) / float(np.max(np.abs(Hw))), pca_ferr2=abs(got["ferr2"] - ora["ferr2"]))
    if ora["eigenvalues"] is not None:
        d["eigenvalues"] = float(np.max(np.abs(np.asarray(got["eigenvalues"]) - ora["eigenvalues"]) / ora["eigenvalues"]))
    return d


def twin_pca(case):
    data, nb = case["data"], case["num_bases"]
    d64 = data.astype(np.float64)
    if case["user_w"] is not None:
        W, ev = case["user_w"], None
    else:
        U, S, _ = twin_svd(data, nb if nb > 0 else -1)
        W = U[:, :nb] if nb > 0 else U
        ev = np.diag(S)[:W.shape[1]]
    H = np.dot(W.T, d64)
    return dict(W=W, H=H, eigenvalues=ev, ferr2=ferr2_identity(data, W, H))


def measure():
    """The largest deviation of the twin from the oracle over all cases, per quantity."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for name in SVD_CASES:
        c = svd_case(name)
        for q, v in svd_deviation(c, twin_svd(c["data"], c["k"])).items():
            worst[q] = max(worst[q], v)
    for name in PCA_CASES:
        c = pca_case(name)
        for q, v in pca_deviation(c, twin_pca(c)).items():
            worst[q] = max(worst[q], v)
    return worst


def tolerances():
    """The committed oracle-vs-twin figures (tests/golden/svd_sparse_tolerances.json, written by gen_golden_svd_sparse.py)."""
    with open(TOL_PATH) as f:
        return json.load(f)["measured"]


def device_tol(quantity):
    t = FACTOR * tolerances()[quantity]
    if quantity in ("U", "V", "W", "H"):
        return max(t, VECTOR_FLOOR)
    if quantity in ("ferr2", "pca_ferr2"):
        return max(t, FERR2_FLOOR)
    return t
