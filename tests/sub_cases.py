"""Shared cases of the column gather (pmf_set_v_gather_f32) and of SUB: built from seeds on the CPU, no device needed.
tests/test_sub_cases.py checks them; tests/test_gpu_gather.py and tests/test_gpu_sub.py run them."""
import numpy as np

# ---- the gather -------------------------------------------------------------------------------------------------------------
# k_gather_cols tiles the destination [mp][np] (np = nsel rounded up to 64 columns; some widths further on NMF contexts) by
# workgroups of 256 threads laid out tx x ty: a thread owns 4 adjacent columns, tx = 16 (np < 256), 64 (np < 1024) or 256 threads
# lie along the row, ty = 16, 4 or 1 rows are written at a time and a workgroup takes a multiple of 4 ty rows.
ROWS = (1, 29, 64, 65, 300)
SRC_COLS = (3, 300, 5000)
NSEL = (1, 3, 16, 17, 64, 65, 130)
# extra destination widths, each across a boundary of that tiling:
NSEL_EXTRA = (
    200,     # np = 256: the first width on tx = 64 (one workgroup along the row, filled exactly)
    260,     # np = 320: tx = 64, the row crosses from the first workgroup (columns 0..255) into a second, partly filled one
    1000,    # np = 1024: the first width on tx = 256 (one workgroup along the row, filled exactly)
    1030,    # np = 1088: tx = 256, the row crosses the workgroup boundary at column 1024
)
# rows 65 and 300 already put a column across the row boundary of a workgroup (mp = 128 and 320 against 64 rows per trip at
# tx = 16); 300 rows at tx = 256 (4 rows per trip) end in a partial trip of the padded rows.
PATTERNS = ("ascending", "descending", "random_repeats", "one_column", "ends")
# a destination of another family: an NMF context with num_bases <= 32 pads 448 columns to 512 (the one-pass kernel's panel
# count), so the pad is wider than 64 columns and the leading dimensions of a whole copy differ
NMF_PADDED = dict(rows=29, n=448, nsel=400, num_bases=4)

SPECIALS = np.array([0x7FC00001, 0x7F800123, 0xFFC0BEEF, 0x7FFFFFFF,      # NaNs with distinct payloads (quiet, signalling, negative)
                     0x7F800000, 0xFF800000,                                # +inf, -inf
                     0x80000000], dtype=np.uint32)                         # -0.0


def gather_data(rows, n, seed=None):
    """rows x n random float32 with the special values at fixed places (as many as fit)."""
    rng = np.random.RandomState(1000 * rows + n if seed is None else seed)
    V = rng.standard_normal((rows, n)).astype(np.float32)
    flat = V.reshape(-1).view(np.uint32)
    for i, bits in enumerate(SPECIALS):
        flat[(i * 7919 + 1) % flat.shape[0]] = bits
    return V


def gather_index(pattern, n, nsel, seed=0):
    """int64 [nsel] in [0, n).  'ascending' / 'descending' are strictly monotone where nsel <= n and repeat neighbours beyond;
    'random_repeats' holds at least one repeat for nsel >= 2; 'ends' holds column n - 1 and, for nsel >= 2, column 0."""
    rng = np.random.RandomState(7 * n + 13 * nsel + seed)
    if pattern == "ascending":
        idx = (np.arange(nsel, dtype=np.int64) * n) // nsel
    elif pattern == "descending":
        idx = ((np.arange(nsel, dtype=np.int64) * n) // nsel)[::-1].copy()
    elif pattern == "random_repeats":
        idx = rng.randint(0, n, size=nsel).astype(np.int64)
        if nsel >= 2:
            idx[nsel // 2] = idx[0]
    elif pattern == "one_column":
        idx = np.full(nsel, n // 2, dtype=np.int64)
    elif pattern == "ends":
        idx = rng.randint(0, n, size=nsel).astype(np.int64)
        idx[-1] = 0
        idx[0] = n - 1
    else:
        raise ValueError(pattern)
    return idx


def gather_cases(rows, n):
    """(nsel, pattern, idx) for one source shape: the issue's grid and the extra widths."""
    for nsel in NSEL + NSEL_EXTRA:
        for pattern in PATTERNS:
            yield nsel, pattern, gather_index(pattern, n, nsel)


# ---- SUB ----------------------------------------------------------------------------------------------------------------------
COMPOSITION_SHAPE = (29, 300)
COMPOSITION = dict(nsub=20, num_bases=4)
UPLOAD_SHAPE = (64, 5000)


def sub_data(rows, n, seed=11):
    """Non-negative float32 data (every mfmethod of the composition test takes it); no zero column."""
    return (np.random.RandomState(seed).random_sample((rows, n)) + 0.05).astype(np.float32)


# 'cur' cases: (rows, n, nsub, seed of np.random).  For each seed every one of the nsub draws lies farther than 1e-9 from the
# nearest cumulative boundary (tests/test_sub_cases.py), so the drawn indices do not depend on the summation order of the norms.
CUR_CASES = (
    (29, 300, 20, 3),
    (64, 5000, 20, 5),
    (2, 3, 2, 1),
)
CUR_MARGIN = 1e-9


def cur_reference(V, nsub, seed):
    """(indices, smallest distance of a draw to a cumulative boundary): sub.py:124-141 in float64 NumPy on the float32-rounded
    data, the draws from np.random seeded with `seed`."""
    d = np.asarray(V, dtype=np.float32).astype(np.float64)
    pcol = (d ** 2).sum(axis=0)
    pcol /= pcol.sum()
    cum = np.cumsum(pcol.flatten())
    np.random.seed(seed)
    idx = np.zeros(nsub, np.int32)
    margin = np.inf
    for i in range(nsub):
        r = np.random.rand()
        idx[i] = np.where(cum >= r)[0][0]
        margin = min(margin, float(np.min(np.abs(cum - r))))
    return np.sort(idx), margin
