"""Cases of tests/test_gpu_snmf_csr.py: SNMF on CSR data, every kernel form of pmf_csr.h on structured sparsity.

Three parts, all on the CPU:
  builders    CSR arrays from a list of row lengths (csr_from_row_lengths), the same matrix with repeated entries
              (with_duplicates) or with the entries of every row permuted (shuffled_rows);
  the atlas   named row-length lists that realise the block structures the kernels branch on -- 16-row blocks around the
              64 entries kept in registers, 64-row blocks around GRAM_CAP = 256, partial last blocks, nothing at all,
              all entries in one column, and matrices deep enough that a wave passes several blocks;
  dispatch    a model of which instantiation the host code launches for (n, num_bases), the list of reachable forms with
              a smallest (n, k) each, and the float64 reference of one step.
tests/test_snmf_csr_cases.py holds every claim made here to the sources and to SciPy."""
import os
import re

import numpy as np
import scipy.sparse as sp

from oracle.snmf_oracle import snmf_update_h

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_SNMF_H = os.path.join(ROOT, "pymf_amd", "csrc", "pmf_host_snmf.h")

GRAM_CAP = 256          # pmf_csr.h: entries of a 64-row block that k_csr_gram stages per wave
GRAM_WAVES = 8
LDS_BYTES = 160 * 1024
MI355X_CUS = 256
U24 = 2.0 ** -24        # unit roundoff of float32


# ---- builders ----------------------------------------------------------------------------------------------------------
def _coprime_strides(n):
    return np.array([s for s in range(1, max(n, 2)) if np.gcd(s, n) == 1] or [1], dtype=np.int64)


def csr_from_row_lengths(n, lengths, seed, cols="random"):
    """(indptr int64, indices int32, data float32) of a len(lengths) x n matrix with lengths[r] entries in row r: columns
    distinct and ascending within a row, values uniform in (-0.3, 0.7) and none zero.
    cols: "random"   start + stride * j mod n with a seeded start and a stride coprime to n per row (distinct for any length
                     up to n, spread over all column tiles);
          "first"    columns 0 .. L - 1;   "last"   columns n - L .. n - 1;   "tile:<j>"   columns 16 j .. inside tile j."""
    lengths = np.asarray(lengths, dtype=np.int64)
    rs = np.random.RandomState(seed)
    m = lengths.shape[0]
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    nnz = int(indptr[-1])
    row = np.repeat(np.arange(m, dtype=np.int64), lengths)
    pos = np.arange(nnz, dtype=np.int64) - indptr[row]
    if cols == "random":
        width, lo = n, 0
        strides = _coprime_strides(n)
        start = rs.randint(0, n, size=m).astype(np.int64)
        stride = strides[rs.randint(0, strides.shape[0], size=m)]
        col = (start[row] + stride[row] * pos) % n
    elif cols == "first":
        width, lo = n, 0
        col = pos
    elif cols == "last":
        width, lo = n, 0
        col = n - lengths[row] + pos
    elif cols.startswith("tile:"):
        lo = 16 * int(cols[5:])
        width = min(16, n - lo)
        col = lo + pos
    else:
        raise ValueError(cols)
    assert lengths.min(initial=0) >= 0 and lengths.max(initial=0) <= width, (cols, n, int(lengths.max(initial=0)))
    order = np.lexsort((col, row))
    indices = col[order].astype(np.int32)
    data = (rs.random_sample(nnz) - 0.3).astype(np.float32)
    data[data == 0] = np.float32(0.5)
    return indptr, indices, data


def with_duplicates(csr, every):
    """The same matrix with every `every`-th stored entry split into two entries of half the value (exact in float32), the
    second placed at the end of its row: repeated (row, column) pairs, and rows whose columns no longer ascend."""
    indptr, indices, data = csr
    nnz = indices.shape[0]
    row = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    pick = np.arange(0, nnz, every)
    half = data.copy()
    half[pick] = half[pick] * np.float32(0.5)
    assert np.all(half[pick] * np.float32(2.0) == data[pick])
    r2 = np.concatenate([row, row[pick]])
    order = np.argsort(r2, kind="stable")                 # the repeats follow the row's own entries
    ip = np.zeros_like(indptr)
    np.cumsum(np.bincount(r2, minlength=indptr.shape[0] - 1), out=ip[1:])
    return ip, np.concatenate([indices, indices[pick]])[order], np.concatenate([half, half[pick]])[order]


def shuffled_rows(csr, seed=0):
    """The same matrix with the stored entries of every row in a seeded random order."""
    indptr, indices, data = csr
    row = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))
    order = np.lexsort((np.random.RandomState(seed).random_sample(indices.shape[0]), row))
    return indptr.copy(), indices[order], data[order]


def as_scipy(csr, n, dtype=np.float64):
    """scipy's CSR matrix of the arrays as they are (no canonicalisation: toarray() and products add repeated entries up)."""
    indptr, indices, data = csr
    return sp.csr_matrix((data.astype(dtype), indices, indptr), shape=(indptr.shape[0] - 1, n))


def block_counts(indptr, rows):
    """Stored entries per block of `rows` consecutive rows (the last block may be partial)."""
    indptr = np.asarray(indptr)
    m = indptr.shape[0] - 1
    edges = np.minimum(np.arange(0, m + rows, rows), m)
    return np.diff(indptr[edges])


def block16_counts(indptr):
    return block_counts(indptr, 16)


def block64_counts(indptr):
    return block_counts(indptr, 64)


# ---- the atlas ---------------------------------------------------------------------------------------------------------
def _spread(count, rows):
    return [count // rows + (1 if i < count % rows else 0) for i in range(rows)]


def _packed(count, rows, n, at_end):
    """count entries in as few rows of n as possible; the rows sit in the middle of the block (rows 0 and rows - 1 empty) or,
    at_end, at its end (row 0 empty, the last row full)."""
    full = [n] * (count // n) + ([count % n] if count % n else [])
    assert len(full) <= rows - 2 or (at_end and len(full) <= rows - 1), (count, n)
    before = rows - len(full) if at_end else (rows - len(full)) // 2
    return [0] * before + full + [0] * (rows - before - len(full))


BLOCKS16_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 200)


def blocks16_lengths(n):
    """18 consecutive 16-row blocks: each count of BLOCKS16_COUNTS once spread evenly over the rows, once packed into as few
    rows as n allows."""
    out = []
    for c in BLOCKS16_COUNTS:
        out += _spread(c, 16)
    for q, c in enumerate(BLOCKS16_COUNTS):
        out += _packed(c, 16, n, at_end=bool(q & 1))
    return out


GRAM_CAP_T = (0, 255, 256, 257, 40, 300, 400, 10, 0, 256, 100)   # the edges of GRAM_CAP, then short long long short empty long short


def gram_cap_lengths(n):
    """Consecutive 64-row blocks with GRAM_CAP_T entries; for n >= 255 one more whose 255 entries sit in a single row (the upper
    end of the byte that k_csr_gram keeps per row length)."""
    out = []
    for t in GRAM_CAP_T:
        out += _spread(t, 64)
    if n >= 255:
        out += [0] * 31 + [255] + [0] * 32
    return out


RAGGED_M = (1, 15, 17, 63, 65, 129)


def pass_geometry(m, n, cus=MI355X_CUS):
    """(workgroups, blocks per wave, waves with one block more) of the pass-per-iteration launch (snmf_csr_fused_iteration,
    with the slab count of pmf_ctx_create)."""
    mp, npad = -(-m // 64) * 64, -(-n // 64) * 64
    blocks16 = mp // 16
    nchunks = min(max(1, 1024 // (-(-npad // 256))), blocks16)
    rpc = -(-(-(-blocks16 // nchunks)) // 4) * 4 * 16
    nchunks = -(-mp // rpc)
    wgs = min(-(-blocks16 // 4), cus, nchunks)
    return wgs, blocks16 // (4 * wgs), blocks16 % (4 * wgs)


def deep_rows(n, cus=MI355X_CUS):
    """A ragged m (the first on a coarse search grid) at which every wave of the pass-per-iteration launch passes three blocks
    or more and some pass one more (blk_extra != 0)."""
    m = 16 * 12 * 8 + 7
    while True:
        wgs, per, extra = pass_geometry(m, n, cus)
        if per >= 3 and extra != 0:
            return m
        m += 16 * 4 * max(1, wgs // 8)


def deep_lengths(n, cus=MI355X_CUS, density=0.01, seed=0):
    """deep_rows(n) rows at about `density`; the first rows are blocks16_lengths(n), so that the waves at the start of the grid
    pass blocks of more than 64 entries one after the other."""
    m = deep_rows(n, cus)
    rs = np.random.RandomState(seed)
    lengths = rs.binomial(n, density, size=m)
    head = blocks16_lengths(n)
    lengths[:len(head)] = head
    return lengths


GRAM_DEEP_PATTERN = (40, 300, 400, 10, 0, 256, 100)      # per wave: short long long short empty long short


def gram_deep_lengths(n):
    """Every wave of k_csr_gram passes GRAM_DEEP_PATTERN: blocks per wave = its length, no remainder.  With the images of C in
    global memory (np >= 192) the launch has 32 workgroups of GRAM_WAVES waves."""
    assert gram_wgs(n) == 32
    one = []
    for t in GRAM_DEEP_PATTERN:
        one += _spread(t, 64)
    return one * (32 * GRAM_WAVES)


def gram_wgs(n):
    npad = -(-n // 64) * 64
    return 256 if 2 * (npad * (npad + 1) // 2) * 8 + GRAM_WAVES * (GRAM_CAP * 9 + 64 * 4 + 64) <= LDS_BYTES else 32


def atlas(n, cus=MI355X_CUS):
    """{name: (row lengths, cols)} of every structure that exists at n columns (SKIPPED lists what does not)."""
    out = {"blocks16": (blocks16_lengths(n), "random"),
           "gram_cap": (gram_cap_lengths(n), "random"),
           "empty": ([0] * 100, "random"),
           "edge_col0": ([1, 0, 1, 1] * 40 + [1] * 7, "first"),
           "edge_collast": ([1, 1, 0, 1] * 40 + [1] * 7, "last"),
           "edge_tile": (_spread(200, 16) + [0] * 16 + _spread(70, 16) + [3, 0, 5], "tile:%d" % ((n - 1) // 16 // 2)),
           "deep": (deep_lengths(n, cus), "random")}
    for m in RAGGED_M:
        out["ragged_m%d" % m] = ([(3 * r + m) % 5 for r in range(m)], "random")
    return out


SMALL = ("blocks16", "gram_cap", "empty", "edge_col0", "edge_collast", "edge_tile") + tuple("ragged_m%d" % m for m in RAGGED_M)
# structures that cannot exist: (what, columns at which it is left out, why)
SKIPPED = [("gram_cap: 255 entries in one row", "n < 255", "a row holds at most n distinct columns"),
           ("edge_tile: 16 columns wide", "last tile of n % 16 != 0", "the tile chosen is an inner one, whole at every n used")]


def build(name, n, cus=MI355X_CUS, seed=1):
    lengths, cols = atlas(n, cus)[name] if name != "gram_deep" else (gram_deep_lengths(n), "random")
    return csr_from_row_lengths(n, lengths, seed=seed + len(lengths), cols=cols)


# ---- which kernel runs -------------------------------------------------------------------------------------------------
def mfma_table():
    """[(NT, NTP)] as csr_mfma() in pmf_host_snmf.h lists them."""
    with open(HOST_SNMF_H) as f:
        src = f.read()
    body = src[src.index("bool csr_mfma("):]
    body = body[:body.index("\n}\n")]
    cases = re.findall(r"case (\d+): \*rc = launch_csr_mfma<(\d+), (\d+)>", body)
    assert cases and all(int(key) == 100 * int(nt) + int(ntp) for key, nt, ntp in cases), cases
    assert len(cases) == len(re.findall(r"\bcase\b", body))
    return [(int(nt), int(ntp)) for _, nt, ntp in cases]


MFMA_TABLE = ((8, 8), (4, 8), (4, 4), (2, 8), (1, 8), (1, 4))       # held to mfma_table() by test_snmf_csr_cases.py


def dispatch(n, k, m=None, cus=MI355X_CUS):
    """What the host code launches for SNMF on CSR data of n columns at k bases (pmf_ctx_create, pmf_set_v_csr_f32,
    snmf_csr_fused_iteration, csr_ps, launch_csr_w_blocks, ensure_vgram)."""
    npad = -(-n // 64) * 64
    nt = 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8
    kp = 16 * nt
    d = dict(NT=nt, KP=kp, np=npad, dense=k > 128 or npad * kp * 4 > LDS_BYTES)
    if d["dense"]:
        return d
    fused_ok = (2 * npad * kp + 4 * 16 * kp) * 4 <= LDS_BYTES
    if not fused_ok:
        d["pass"] = None                                   # the hooks: k_csr_w_blocks, then k_csr_p
    elif (nt, npad // 16) in MFMA_TABLE:
        d["pass"] = "k_snmf_csr_mfma<%d,%d>" % (nt, npad // 16)
    else:
        d["pass"] = "k_snmf_csr_fused<%d>" % nt
        ns = nt * (nt + 1) // 2
        d["one_region"] = 2 * ns * 1024 > npad * kp * 4
    d["p"] = "k_csr_p<%d>" % (1 if kp <= 64 else 2)
    d["w"] = "k_csr_w_blocks<%d>" % nt
    d["w_m_in_lds"] = npad * kp * 4 <= 128 * 1024
    if m is not None:
        d["w_persistent"] = not ((-(-m // 64) * 64 // 16 + 15) // 16 >= 8 * cus)
    d["gram"] = npad <= 1024
    d["gram_image"] = "lds" if gram_wgs(n) == 256 else "global"
    return d


# (what is meant to run, n, k): the smallest shapes of every reachable form
PASS_FORMS = [("k_snmf_csr_mfma<1,4>", 50, 7), ("k_snmf_csr_mfma<4,4>", 64, 33), ("k_snmf_csr_mfma<1,8>", 100, 16),
              ("k_snmf_csr_mfma<2,8>", 128, 17), ("k_snmf_csr_mfma<4,8>", 96, 40), ("k_snmf_csr_mfma<8,8>", 128, 65),
              ("k_snmf_csr_fused<1>", 192, 9), ("k_snmf_csr_fused<1>", 1100, 5),
              ("k_snmf_csr_fused<2>", 64, 20), ("k_snmf_csr_fused<2>", 192, 24), ("k_snmf_csr_fused<4>", 192, 40)]
P_FORMS = [("k_csr_p<1>", 320, 64), ("k_csr_p<2>", 192, 70)]
W_FORMS = [("k_csr_w_blocks<1>", True, 50, 7), ("k_csr_w_blocks<2>", True, 64, 20), ("k_csr_w_blocks<4>", True, 96, 40),
           ("k_csr_w_blocks<8>", True, 128, 65),                                              # (.., M in LDS, n, k)
           # M through L2: np KP 4 bytes beyond 128 KiB, within the 160 KiB up to which the rows stay CSR
           ("k_csr_w_blocks<1>", False, 2100, 7), ("k_csr_w_blocks<2>", False, 1100, 20), ("k_csr_w_blocks<4>", False, 600, 40),
           ("k_csr_w_blocks<8>", False, 320, 100)]
GRAM_FORMS = [("lds", 50, 7), ("lds", 128, 33), ("global", 255, 20)]                           # np <= 128 | np = 256 (n = 255: a row of 255 entries exists)


def reachable():
    return ([("pass",) + f for f in PASS_FORMS] + [("p",) + f for f in P_FORMS] +
            [("w", name + ("/lds" if lds else "/l2"), n, k) for name, lds, n, k in W_FORMS] +
            [("gram", image, n, k) for image, n, k in GRAM_FORMS])


def dead_forms(max_n=1300):
    """The (kernel, n, k) with k <= n that would run k_snmf_csr_fused<8> or the one-region branch of its S exchange: none."""
    out = []
    for n in range(1, max_n + 1):
        for k in (1, 16, 17, 32, 33, 64, 65, 128):
            if k > n:
                continue
            d = dispatch(n, k)
            if d.get("pass") == "k_snmf_csr_fused<8>" or d.get("one_region"):
                out.append((d["pass"], n, k))
    return out


# ---- the reference -----------------------------------------------------------------------------------------------------
def h0(n, k, seed=0):
    return (np.random.RandomState(1000 * k + n + seed).random_sample((k, n)) + 0.05).astype(np.float32)


def reference_step(csr, n, H):
    """One SNMF iteration from H in float64 on the matrix the arrays describe: M = H^T inv(H H^T), W = V M as a sparse product
    (the dense product on toarray() gives the same to float64 rounding: test_snmf_csr_cases.py), H through the oracle's
    update_h.  Returns (M, W, H)."""
    H = np.array(H, dtype=np.float64)
    V = as_scipy(csr, n)
    M = np.dot(H.T, np.linalg.inv(np.dot(H, H.T)))
    W = np.asarray(V @ M)
    return M, W, snmf_update_h(V, W, H.copy())


def w_bound(csr, n, M, W):
    """Componentwise bound of |W_dev - W| for W[r, :] = sum_e v_e M32[col_e, :] in float32: M rounded once, at most L_r fused
    multiply-adds on row r -- (L_r + 3) 2^-24 (|V| |M|)[r, :], plus one ulp of the result."""
    indptr, indices, data = csr
    L = np.diff(indptr).astype(np.float64)
    A = sp.csr_matrix((np.abs(data).astype(np.float64), indices, indptr), shape=(indptr.shape[0] - 1, n))
    absprod = np.asarray(A @ np.abs(M))
    return (L[:, None] + 3.0) * U24 * absprod + np.spacing(np.abs(W).astype(np.float32)).astype(np.float64) * (absprod > 0)


def w_ratio(csr, n, M, W, Wdev):
    """max |W_dev - W| / bound over the rows with entries (<= 1 passes); rows without entries must be exactly 0.0."""
    Wdev = np.asarray(Wdev, dtype=np.float64)
    emptyrow = np.diff(csr[0]) == 0
    assert np.all(Wdev[emptyrow] == 0.0), "a row without entries is not exactly zero"
    b = w_bound(csr, n, M, W)
    err = np.abs(Wdev - W)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0
