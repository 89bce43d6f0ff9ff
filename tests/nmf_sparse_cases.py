"""The cases of NMF on scipy.sparse data (k_nmf_sp_step, pmf_nmf_csr.h), defined once: data, start states and float64 oracle
runs (oracle.NMFOracle on toarray()), each computed once and shared by tests/test_nmf_sparse_cases.py (no GPU: the cases
leave room for float32) and tests/test_gpu_nmf_sparse.py.

Corners of the kernel: every width (NT = 1, 2, 4, 8) at its lowest and highest k; a shape below one 64-row pad (37 x 29), one
whose H step has more rows than one workgroup takes and whose n is the size at which the SNMF CSR path expands to dense
(1003 x 520), one with several workgroups and a slab sum in the W step (5000 x 300); and CORNER, a matrix with empty rows and
columns, rows of exactly 63, 64, 65 and 300 stored entries in one 16-row block (the first 64 entries of a block travel in
registers, the rest come straight from memory), stored explicit zeros and unsummed duplicates."""
import collections
import functools

import numpy as np
import scipy.sparse as sp

import oracle

TOL = 2e-5                      # relative Frobenius error of W and of H for NMF
NITER = 3

Case = collections.namedtuple("Case", "m n k density seed")

KS = (1, 16, 17, 32, 33, 64, 65, 128)
SHAPES = ((37, 29, 0.3), (1003, 520, 0.02), (5000, 300, 0.01))
WIDTH_CASES = [Case(m, n, k, d, 7) for (m, n, d) in SHAPES for k in KS]

LOOP_CASE = Case(1003, 520, 33, 0.02, 7)        # loop forms, reproducibility, data handling
LOOP_NITER = 6
ABI_CASE = Case(1003, 520, 100, 0.02, 7)        # the C ABI alone, at the golden's width

CORNER = Case(130, 320, 20, 0.05, 9)
CORNER_EMPTY_ROWS = (0, 17, 129)
CORNER_EMPTY_COLS = (0, 7, 319)
CORNER_LONG_ROWS = {3: 63, 4: 64, 5: 65, 6: 300}


def case_id(c):
    return "%dx%d-k%d" % (c.m, c.n, c.k)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def f32_values(rs, size):
    """float64 values that float32 holds exactly, in [0.05, 1.05)"""
    return (rs.random_sample(size) + 0.05).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def matrix(c):
    """The data as a canonical CSR matrix (float64 holding float32-representable values)."""
    if c == CORNER:
        return corner_formats()["canonical"]
    rs = np.random.RandomState(c.seed)
    V = sp.random(c.m, c.n, density=c.density, format="csr", random_state=rs, data_rvs=lambda size: f32_values(rs, size))
    V.sum_duplicates()
    return V


@functools.lru_cache(maxsize=None)
def corner_triplets():
    """(rows, cols, vals) in row order with duplicates (rows 40 .. 59) and explicit zeros (rows 60 .. 79) among them."""
    c = CORNER
    rs = np.random.RandomState(c.seed)
    cols_ok = np.setdiff1d(np.arange(c.n), CORNER_EMPTY_COLS)
    rows, cols, vals = [], [], []
    for r in range(c.m):
        if r in CORNER_EMPTY_ROWS:
            continue
        cnt = CORNER_LONG_ROWS.get(r, 1 + rs.randint(0, 2 * int(c.density * c.n)))
        cc = np.sort(rs.choice(cols_ok, size=cnt, replace=False))
        vv = f32_values(rs, cnt)
        if 40 <= r < 60:                        # every entry of these rows is stored twice, with two different values
            cc = np.repeat(cc, 2)
            vv = np.round(np.stack([vv, f32_values(rs, cnt)], axis=1).reshape(-1) * 4096.0) / 4096.0   # (their sums are exact in float32)
        if 60 <= r < 80:
            vv[::3] = 0.0                       # stored zeros
        rows.append(np.full(len(cc), r)); cols.append(cc); vals.append(vv)
    return frozen(np.concatenate(rows), np.concatenate(cols).astype(np.int64), np.concatenate(vals))


@functools.lru_cache(maxsize=None)
def corner_formats():
    """The corner matrix as the caller may hand it over: raw CSR (duplicates unsummed), COO, CSC; and its canonical CSR."""
    c = CORNER
    rows, cols, vals = corner_triplets()
    indptr = np.zeros(c.m + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    indptr = np.cumsum(indptr)
    raw = sp.csr_matrix((vals.copy(), cols.astype(np.int32), indptr), shape=(c.m, c.n))
    coo = sp.coo_matrix((vals.copy(), (rows.copy(), cols.copy())), shape=(c.m, c.n))
    canonical = raw.copy()
    canonical.sum_duplicates()
    return {"raw_csr": raw, "coo": coo, "csc": canonical.tocsc(), "canonical": canonical}


@functools.lru_cache(maxsize=None)
def start(c):
    """(W0, H0): float64 arrays of float32-representable values."""
    rs = np.random.RandomState(c.seed + 1000)
    return frozen(rs.random_sample((c.m, c.k)).astype(np.float32).astype(np.float64),
                  rs.random_sample((c.k, c.n)).astype(np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def oracle_run(c, niter=NITER, compute_w=True, compute_h=True):
    """(W, H) of oracle.NMFOracle on toarray(), float64."""
    W0, H0 = start(c)
    o = oracle.NMFOracle(matrix(c).toarray(), num_bases=c.k)
    o.W, o.H = W0.copy(), H0.copy()
    o.factorize(niter=niter, compute_w=compute_w, compute_h=compute_h, compute_err=False)
    return frozen(o.W, o.H)


def gather32(c, niter=NITER, compute_w=True, compute_h=True):
    """The gather-form update (pmf_nmf_csr.h) restated in float32 NumPy: X <- X * (V_rows Y) / (X G + 1e-9), G = Y^T Y carried
    over from the half step that wrote Y.  -> (W, H) as float64."""
    V = matrix(c).astype(np.float32)
    Vt = V.T.tocsr()
    W0, H0 = start(c)
    W, Ht = W0.astype(np.float32), np.ascontiguousarray(H0.T.astype(np.float32))
    eps = np.float32(1e-9)
    G_h, G_w = Ht.T.dot(Ht), W.T.dot(W)
    for _ in range(niter):
        if compute_w:
            W = (W * (V.dot(Ht))) / (W.dot(G_h) + eps)
            G_w = W.T.dot(W)
        if compute_h:
            Ht = (Ht * (Vt.dot(W))) / (Ht.dot(G_w) + eps)
            G_h = Ht.T.dot(Ht)
    assert W.dtype == np.float32 and Ht.dtype == np.float32
    return W.astype(np.float64), Ht.T.astype(np.float64)


def geometry(m, n, k):
    """What pmf_ctx_create and the launch of k_nmf_sp_step derive from a shape (256 compute units)."""
    NT = 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8
    waves = 4 if NT == 8 else 8
    mp, np_ = -(-m // 64) * 64, -(-n // 64) * 64
    return dict(NT=NT, KP=16 * NT, mp=mp, np=np_, wgs_w=min(-(-(mp // 16) // waves), 256), wgs_h=min(-(-(np_ // 16) // waves), 256))
