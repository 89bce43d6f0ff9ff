"""Cases of tests/test_gpu_fused_bits.py: every k_nmf_fused instantiation the host dispatch can reach, at the
smallest shapes at which its block loop can still go wrong, and the digests a run of them yields.

Per instantiation two cases:
  full    m = 256 workgroups x 4 waves x 16 rows x 3 blocks (a wave passes its first block, a middle one and its
          last), n = 64 x panels (the upper end of the panel count), k = 16 NT;
  ragged  m = that + 16 x 5 + 7 (some waves take one block more -- blk_extra -- and the last block is partial),
          n = 64 x (panels - 1) + 16 (the lower end), k = 16 NT - 3 (not a multiple of 16).
V, W0 and H0 come from the library's seeded device fills, so a case costs no upload."""
import hashlib
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "fused_bits.json")
FUSED_H = os.path.join(ROOT, "pymf_amd", "csrc", "pmf_fused.h")

M_FULL = 256 * 4 * 16 * 3
M_RAGGED = M_FULL + 16 * 5 + 7
NITER = 3
MODES = ("nmf", "snmf", "bnmf", "rnmf")
ALGO_OF = {"nmf": 0, "snmf": 2, "bnmf": 3, "rnmf": 4}     # _lib.ALGO_*


def dispatch_table():
    """[(NT, NPANEL, SPLIT)] as pmf_fused.h's launch_fused() lists them."""
    with open(FUSED_H) as f:
        src = f.read()
    one = [(int(a), int(b), 1) for a, b in re.findall(r"^\s*PMF_FUSED_CASE\(\d+, (\d+), (\d+)\)", src, re.M)]
    two = [(int(a), int(b), 2) for a, b in re.findall(r"^\s*PMF_FUSED_SPLIT_CASE\(\d+, (\d+), (\d+)\)", src, re.M)]
    return one + two


def kernel_name(nt, npanel, split, mode):
    """The name pmf_path_name() reports (fused_kernel_name in pmf_fused.h)."""
    return "k_nmf_fused<%d,%d%s%s>" % (nt, npanel, "" if mode == "nmf" else "," + mode, ",SPLIT 2" if split == 2 else "")


def instantiations():
    """Every (NT, NPANEL, SPLIT, mode) the host path launches: the one-block-per-wave table in all four modes, the
    two-waves-per-block table in all but SNMF (launch_fused(), fused_grid_for(allow_split = not SNMF))."""
    return [(nt, npanel, split, mode) for nt, npanel, split in dispatch_table() for mode in MODES
            if not (split == 2 and mode == "snmf")]


def cases():
    out = []
    for nt, npanel, split, mode in instantiations():
        panels = npanel * split
        name = kernel_name(nt, npanel, split, mode)
        out.append((name + " full", name, mode, M_FULL, 64 * panels, 16 * nt))
        out.append((name + " ragged", name, mode, M_RAGGED, 64 * (panels - 1) + 16, 16 * nt - 3))
    return out


def run_case(_lib, mode, m, n, k):
    """NITER iterations from the seeded fills through the C ABI -> (path name, sha256 of W, sha256 of H)."""
    ctx = _lib.Context(ALGO_OF[mode], m, n, k)
    try:
        ctx.fill_v_uniform(11)
        ctx.fill_w_uniform(12)
        ctx.fill_h_uniform(13)
        if mode == "bnmf":
            ctx.set_lambda(0.05, 0.05)
        if mode == "rnmf":
            ctx.set_lambda(0.3, 0.0)
            ctx.rnmf_update_s()
        ctx.factorize(NITER)
        W = np.ascontiguousarray(ctx.get_w(), dtype=np.float32)
        H = np.ascontiguousarray(ctx.get_h(), dtype=np.float32)
        return ctx.path_name, hashlib.sha256(W.tobytes()).hexdigest(), hashlib.sha256(H.tobytes()).hexdigest()
    finally:
        ctx.close()
