"""The device cases of SVD and PCA (tests/test_gpu_svd.py) and what makes the comparison with the float64 oracle meaningful
(tests/test_svd_cases.py, no GPU): the smallest shapes at which k_prod_f64 (Gram tile map) and the paths behind it can go wrong.

Data are U0 diag(s) V0^T with random orthonormal U0, V0 and a prescribed geometric spectrum, rounded to float32, so that by
construction every kept eigenvalue of the Gram matrix is far above svd.py's 1e-8 cut, every dropped one far below it, and
adjacent singular values are at least 5 % apart (well-conditioned vectors: only the sign is free).  With a step of 5 % and
the kept eigenvalues within 1e-4 of the largest, at most 94 singular values fit: the two-tile shapes (130 rows or columns)
have rank 90.

k_prod_f64 cuts the inner dimension into chunks of at least PMF_SVD_MIN_CHUNK = 512 (a multiple of 64): 300 columns (padded
to 320) are one chunk, 2 100 (padded to 2 112) four chunks of 576 with a ragged tail of 384.
"""
import json
import os

import numpy as np

import svd_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PATH = os.path.join(HERE, "golden", "svd_tolerances.json")

# name: (rows, cols, rank, seed, largest singular value, step, offset[, constant first singular vectors])
SVD_CASES = {
    "doc_2x3": None,                                           # svd.py:66-72
    "1x5": (1, 5, 1, 41, 3.0, 1.1, 0.0),                       # one row: a 1 x 1 Gram matrix, Jacobi on a padded 2 x 2
    "37x29": (37, 29, 29, 42, 8.0, 1.10, 0.0),                 # left, odd n: Jacobi pads to even
    "29x300": (29, 300, 29, 43, 12.0, 1.10, 0.0),              # right, one tile, one chunk
    "29x2100": (29, 2100, 29, 44, 30.0, 1.10, 0.0),            # right, one tile, four chunks with a ragged tail
    "130x2100": (130, 2100, 90, 45, 30.0, 1.052, 0.0),         # right, two row tiles: an off-diagonal tile and the mirror
    "300x40": (300, 40, 40, 46, 12.0, 1.08, 0.0),              # left, one tile, one chunk
    "2100x130": (2100, 130, 90, 47, 30.0, 1.052, 0.0),         # left, two tiles, four chunks with a ragged tail
    "300x40_rank25": (300, 40, 25, 48, 12.0, 1.10, 0.0),       # dropped eigenvalues
    # lambda_1 = (4200 + 1000 sqrt(29 * 300))^2 >> the rest: float64 accumulation saves the small ones
    "29x300_offset": (29, 300, 29, 49, 4200.0, 1.052, 1000.0, True),
}

# name: (rows, cols, rank, seed, largest singular value, step, num_bases, center_mean); centred cases: constant first singular vectors
PCA_CASES = {
    "doc_2x3_k2": None,                                        # pca.py:51-54
    "300x40_centred": (300, 40, 40, 51, 12.0, 1.08, 0, True),  # centring leaves a null eigenvalue: it must be dropped
    "29x300_k5": (29, 300, 29, 52, 12.0, 1.10, 5, True),
    "37x29_raw": (37, 29, 29, 53, 8.0, 1.10, 0, False),
}

MIN_CHUNK = 512          # PMF_SVD_MIN_CHUNK (pymf_amd/csrc/pmf_svd.h)
TARGET_WGS = 512         # PMF_SVD_TARGET_WGS
MAX_RANK = 2432          # PMF_SVD_MAX_RANK
FACTOR = 4.0             # device tolerance = FACTOR x the oracle-vs-twin deviation
QUANTITIES = ("U", "V", "S", "svd_ferr", "W", "H", "eigenvalues", "ferr")

_DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])


def planted(rows, cols, rank, seed, smax, step, offset=0.0, ones=False):
    """U0 diag(s) V0^T + offset, float32.  ones: the first columns of U0 and V0 are the constant vectors, so that adding a
    constant only raises the first singular value (by offset sqrt(rows cols)) and centring the rows only removes the first
    singular triple: the rest of the prescribed spectrum stays as it is."""
    rng = np.random.RandomState(seed)
    A, B = rng.randn(rows, rank), rng.randn(cols, rank)
    if ones:
        A[:, 0], B[:, 0] = 1.0, 1.0
    U0, V0 = np.linalg.qr(A)[0], np.linalg.qr(B)[0]
    if ones:                                                   # (QR may return the constant columns negated)
        U0[:, 0], V0[:, 0] = np.abs(U0[:, 0]), np.abs(V0[:, 0])
    s = smax / step ** np.arange(rank)
    return (np.dot(U0 * s, V0.T) + offset).astype(np.float32)


def svd_data(name):
    """float32 data of an SVD case."""
    spec = SVD_CASES[name]
    return _DOC.astype(np.float32) if spec is None else planted(*spec)


def pca_data(name):
    """(float64 data holding float32 values, num_bases, center_mean) of a PCA case: the centred array is float64, as the
    reference's, and is rounded to float32 on its way to the device."""
    spec = PCA_CASES[name]
    if spec is None:
        return _DOC.copy(), 2, True
    return planted(*spec[:6], ones=spec[7]).astype(np.float64), spec[6], spec[7]


def chunks(inner_padded, ntiles):
    """(chunks, chunk length) of k_prod_f64 for a padded inner dimension: svd_chunks of pmf_host_svd.h."""
    nch = max(1, min(TARGET_WGS // ntiles, inner_padded // MIN_CHUNK))
    cl = -(-(-(-inner_padded // nch)) // 64) * 64
    return -(-inner_padded // cl), cl


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.asarray(a).size else 0.0


def svd_deviation(data, got, want):
    """Deviation of the (U, S, V) triple `got` from `want` (same rank), signs fixed: U and V by their largest entry (unit
    vectors), S relative, the Frobenius error relative to ||data||."""
    left = data.shape[0] > data.shape[1]
    Ug, Vg = so.fix_svd_signs(got[0], got[2], left)
    Uw, Vw = so.fix_svd_signs(want[0], want[2], left)
    sg, sw = np.diag(got[1]), np.diag(want[1])
    d64 = np.asarray(data, dtype=np.float64)
    return dict(U=max_abs(Ug, Uw), V=max_abs(Vg, Vw), S=float(np.max(np.abs(sg - sw) / sw)),
                svd_ferr=abs(so.svd_ferr(d64, *got) - so.svd_ferr(d64, *want)) / np.linalg.norm(d64))


def fix_pca_signs(W, H, left):
    """Signs fixed on the eigenvector side: the columns of W, or (rows > cols) the rows of H = S V."""
    if left:
        H2, W2 = so.fix_signs(H, W, 1)
        return W2, H2
    return so.fix_signs(W, H, 0)


def pca_deviation(got, want):
    """Deviation of a PCA result dict (W, H, eigenvalues, ferr) from the oracle's `want` (which also carries the centred data):
    W by its largest entry, H relative to its largest entry, eigenvalues relative, ferr relative to ||data||."""
    left = want["data"].shape[0] > want["data"].shape[1]
    Wg, Hg = fix_pca_signs(got["W"], got["H"], left)
    Ww, Hw = fix_pca_signs(want["W"], want["H"], left)
    return dict(W=max_abs(Wg, Ww), H=max_abs(Hg, Hw) / float(np.max(np.abs(Hw))),
                eigenvalues=float(np.max(np.abs(np.asarray(got["eigenvalues"]) - want["eigenvalues"]) / want["eigenvalues"])),
                ferr=abs(float(got["ferr"]) - want["ferr"]) / np.linalg.norm(want["data"]))


_cache = {}


def svd_case(name):
    """dict(data float32, U, S, V, ferr, left): the float64 oracle on the float32-representable data."""
    if ("svd", name) not in _cache:
        data = svd_data(name)
        U, S, V = so.svd(data.astype(np.float64))
        _cache[("svd", name)] = dict(data=data, U=U, S=S, V=V, ferr=so.svd_ferr(data, U, S, V), left=data.shape[0] > data.shape[1])
    return _cache[("svd", name)]


def pca_case(name):
    """dict(data, num_bases, center_mean, oracle): the float64 oracle of one PCA.factorize()."""
    if ("pca", name) not in _cache:
        data, nb, cm = pca_data(name)
        _cache[("pca", name)] = dict(data=data, num_bases=nb, center_mean=cm, oracle=so.pca(data, nb, cm))
    return _cache[("pca", name)]


def measure():
    """The largest deviation of the float32 twin from the oracle over all cases, per quantity."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for name in SVD_CASES:
        c = svd_case(name)
        d = svd_deviation(c["data"], so.svd(c["data"], f32_twin=True), (c["U"], c["S"], c["V"]))
        for q, v in d.items():
            worst[q] = max(worst[q], v)
    for name in PCA_CASES:
        c = pca_case(name)
        d = pca_deviation(so.pca(c["data"], c["num_bases"], c["center_mean"], f32_twin=True), c["oracle"])
        for q, v in d.items():
            worst[q] = max(worst[q], v)
    return worst


def tolerances():
    """The committed oracle-vs-twin figures (tests/golden/svd_tolerances.json, written by tests/golden/gen_golden_svd.py)."""
    with open(TOL_PATH) as f:
        return json.load(f)["measured"]


def device_tol(quantity):
    return FACTOR * tolerances()[quantity]
