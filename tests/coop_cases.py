"""Cases of tests/test_gpu_coop_tiles.py: every k_nmf_coop instantiation the host dispatch can reach, at the smallest
row counts at which a workgroup passes a first, a middle and a last tile (tests/test_coop_cases.py checks, without a
GPU, that the cases are what they claim).

The grid is one workgroup per CU (coop_grid_for) and tiles have 16 RB rows, dealt out as tile_per plus one extra for the
first tile_extra workgroups.  At 256 CUs, mp = 64 x 550 = 35 200 rows are
  RB = 4:   550 tiles, tile_per 2, tile_extra 38;     RB = 2:  1 100 tiles, tile_per 4, tile_extra 76,
so every workgroup prefetches at least one tile beside an S part (the `more` path of the kernel) and some do one more.

Per instantiation two cases:
  full    m = M_FULL, n = 64 PN, k = 64 BT: no pad rows, no pad columns, no pad bases;
  ragged  m = M_RAGGED (same mp, 7 live rows in the last 64), k = 32 BT + 3 (one wave owns a partly padded base range,
          the last wave pad bases only), n at the lower end of what the instantiation takes after the host's padding.
"""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COOP_H = os.path.join(ROOT, "pymf_amd", "csrc", "pmf_coop.h")

M_FULL = 64 * 550
M_RAGGED = 35143
SLICE_ROWS = 8192            # a context of this many rows: one tile per workgroup at 256 CUs
CUS = 256                    # the MI355X; the device tests read the real count
MODES = ("nmf", "bnmf", "rnmf")
ALGO_OF = {"nmf": 0, "bnmf": 3, "rnmf": 4}     # _lib.ALGO_*
CLASS_OF = {"nmf": "NMF", "bnmf": "BNMF", "rnmf": "RNMF"}
RNMF_LAMB = 1.0

# ragged n of the shapes whose lower end is not 64 (PN - 1) + 16: np = 320 is padded to 384 (two whole pad panels),
# np = 448 to 512 (coop_pad_np)
RAGGED_N = {(2, 2, 6): 272, (1, 4, 6): 272, (1, 4, 8): 400}


def dispatch_table():
    """[(BT, RB, PN, modes)] as pmf_coop.h's launch_coop() lists them."""
    with open(COOP_H) as f:
        src = f.read()
    out = []
    for which, bt, rb, pn in re.findall(r"^\s*PMF_COOP_CASE([23])\((\d+), (\d+), (\d+)\)", src, re.M):
        out.append((int(bt), int(rb), int(pn), MODES if which == "3" else MODES[:2]))
    return out


def instantiations():
    """Every (BT, RB, PN, mode) the host path launches."""
    return [(bt, rb, pn, mode) for bt, rb, pn, modes in dispatch_table() for mode in modes]


def kernel_name(bt, rb, pn, mode):
    """The name pmf_path_name() reports (pmf_ctx_create)."""
    return "k_nmf_coop<%d,%d,%d%s>" % (bt, rb, pn, "" if mode == "nmf" else "," + mode)


# ---- the host's rules, restated ----------------------------------------------------------------------------------
def round_up(x, q):
    return (x + q - 1) // q * q


def coop_shape(nt, np_):
    """coop_shape (pmf_coop.h): (BT, RB, PN) or None."""
    if np_ % 64 != 0 or np_ < 64:
        return None
    pn = np_ // 64
    if nt == 8:
        if pn <= 4:
            return (2, 4, pn)
        if pn == 6:
            return (2, 2, pn)
        return None
    if nt == 4:
        if pn in (6, 8):
            return (1, 4, pn)
    return None


def coop_pad_np(nt, np_):
    """coop_pad_np (pmf_coop.h): the padded column count, 0: leave as it is."""
    pn = np_ // 64
    if nt == 8 and 4 < pn <= 6:
        return 384
    if nt == 4 and 4 < pn <= 8:
        return 384 if pn <= 6 else 512
    return 0


def fused_takes(nt, np_):
    """fused_grid_for(...) > 0 (pmf_fused.h): k_nmf_fused covers the shape, so the cooperative kernel is not asked."""
    pn = np_ // 64
    if np_ % 64 == 0 and 1 <= pn <= {1: 6, 2: 5, 4: 4}.get(nt, 0):
        return True
    return (nt == 2 and np_ in (384, 512)) or (nt == 1 and np_ == 512)      # SPLIT 2 (every mode here allows it)


def host_instantiation(mode, n, k):
    """(BT, RB, PN) of the k_nmf_coop instantiation pmf_ctx_create chooses for (algo, n, k), None where it chooses
    another path: the np / NT rules, coop_pad_np for NMF and BNMF, RNMF only when bt == 2 and rb == 4."""
    if k > 128:
        return None
    nt = 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8
    np_ = round_up(n, 64)
    if mode in ("nmf", "bnmf"):
        if nt <= 2 and np_ == 448:
            np_ = 512
        padded = coop_pad_np(nt, np_)
        if padded > 0:
            np_ = padded
    if fused_takes(nt, np_):
        return None
    shape = coop_shape(nt, np_)
    if shape is None:
        return None
    if mode == "rnmf" and not (shape[0] == 2 and shape[1] == 4):
        return None
    return shape


def tiles(m, rb, cus=CUS):
    """(ntiles, wgs, tile_per, tile_extra) of a context of m rows (pmf_ctx_create, coop_grid_for, launch_coop_t)."""
    mp = round_up(m, 64)
    ntiles = mp // (16 * rb)
    wgs = min(ntiles, cus)
    return ntiles, wgs, ntiles // wgs, ntiles % wgs


def tile_position(tile, m, rb, cus=CUS):
    """(workgroup b, its first tile t0, tt = position of `tile` in b's loop, ntile of b): k_nmf_coop's own deal."""
    _, wgs, per, extra = tiles(m, rb, cus)
    edge = extra * (per + 1)
    b = tile // (per + 1) if tile < edge else extra + (tile - edge) // per
    t0 = b * per + min(b, extra)
    return b, t0, tile - t0, per + (1 if b < extra else 0)


def ndma(bt, rb, pn):
    """NDMA of k_nmf_coop: LDS-DMA instructions per wave and tile."""
    return rb * (64 * bt // 16 + 4 * pn) // 4


def dma_beside_s(bt, rb):
    """DMA slots beside the S part's MFMAs (two per step, RB x BT x 4 steps); what exceeds them goes out at once."""
    return rb * bt * 4 * 2


# ---- the cases ---------------------------------------------------------------------------------------------------
def cases():
    """[(id, kernel name, (BT, RB, PN), mode, kind, m, n, k)]"""
    out = []
    for bt, rb, pn, mode in instantiations():
        name = kernel_name(bt, rb, pn, mode)
        out.append((name + " full", name, (bt, rb, pn), mode, "full", M_FULL, 64 * pn, 64 * bt))
        n = RAGGED_N.get((bt, rb, pn), 64 * (pn - 1) + 16)
        out.append((name + " ragged", name, (bt, rb, pn), mode, "ragged", M_RAGGED, n, 32 * bt + 3))
    return out


def ragged_cases():
    return [c for c in cases() if c[4] == "ragged"]


def case_by_id(cid):
    return next(c for c in cases() if c[0] == cid)


def inputs(case):
    """(V float32, W0, H0 float64 holding float32 values), seeded on the case."""
    cid, _, (bt, rb, pn), mode, kind, m, n, k = case
    seed = 1000 * (100 * bt + 10 * rb + pn) + 10 * MODES.index(mode) + (kind == "ragged")
    rs = np.random.RandomState(seed)
    V = rs.random_sample((m, n)).astype(np.float32)
    if mode == "bnmf":
        V = (V < 0.3).astype(np.float32)
    if mode == "rnmf":
        V.flat[rs.randint(0, V.size, size=V.size // 300)] += 5.0
    W0 = rs.random_sample((m, k)).astype(np.float32).astype(np.float64)
    H0 = rs.random_sample((k, n)).astype(np.float32).astype(np.float64)
    return V, W0, H0
