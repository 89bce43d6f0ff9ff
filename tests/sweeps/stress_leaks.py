#!/usr/bin/env python3
"""Long loops and many contexts: device memory and host RSS must come back (leak check), results must stay finite."""
import os, sys, time, resource
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import ctypes
import pymf_amd
from pymf_amd import _lib
from pymf_amd.rnmf import RNMF

hip = ctypes.CDLL("libamdhip64.so")


def free_mib():
    f, t = ctypes.c_size_t(), ctypes.c_size_t()
    hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t))
    return f.value / 2**20


def rss_mib():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


rs = np.random.RandomState(0)
V = rs.random_sample((4096, 256)).astype(np.float32)
bad = 0
# The added cases are sized so that the buffers only THEY own, leaked once per context, pass the 64 MiB threshold within the 55
# counted repetitions (> 1.2 MiB per context; the large ones named here are >= 2 MiB each):
#   BNMF 4096 x 256, 128 bases: dW1 2 MiB                      RNMF 4096 x 256: dD 4 MiB
#   NMFNNLS 65536 x 256: dW1 4 MiB                             streamed NMF 8192 x 256, tiles of 2048 rows: dTile[2] 2 MiB each
#   CNMF 256 x 2048, 128 bases: dGT dCnA dCnB dCnHn dCnHp 2 MiB each, dC 32 MiB
#   SNMF 4096 x 2048, 128 bases, snapshots: dWsnap 2 MiB, dHsnap 5 MiB, dHdSnap 2 MiB
#   SNMF on CSR 262144 x 256, 2 % non-zeros: dIndptr 2 MiB, dIndices and dVals 5 MiB each
Vtall = rs.random_sample((65536, 256)).astype(np.float32)
Vwide = rs.random_sample((256, 2048)).astype(np.float32)
Vsnap = rs.random_sample((4096, 2048)).astype(np.float32) - 0.5
try:
    import scipy.sparse as sp
    Vcsr = sp.random(262144, 256, density=0.02, format="csr", dtype=np.float32, random_state=rs)
    Vcsr.data -= 0.5
except ImportError:
    Vcsr = None
    print("scipy is not importable: the SNMF-on-CSR case is skipped")


def plain(cls, data, k=16, **kw):
    def run():
        mdl = cls(data, num_bases=k)
        mdl.factorize(niter=3, **kw)
        return mdl
    return run


def streamed():                 # V never resident: row tiles through the two tile buffers
    mdl = pymf_amd.NMF(Vtall[:8192], num_bases=16)
    mdl.stream_rows = 2048
    mdl.factorize(niter=3)
    return mdl


def snmf_snapshots():           # a second call on device-only factors: W is copied device to device first; then both snapshot buffers by name
    mdl = pymf_amd.SNMF(Vsnap, num_bases=128)
    mdl.factorize(niter=2)
    mdl.factorize(niter=2)
    mdl._ctx.snapshot_w(); mdl._ctx.snapshot_h()
    return mdl


cases = [plain(pymf_amd.NMF, V), plain(pymf_amd.SNMF, V - 0.5), plain(pymf_amd.NMFALS, V), plain(pymf_amd.BNMF, V, k=128),
         plain(RNMF, V), plain(pymf_amd.CNMF, Vwide, k=128), plain(pymf_amd.NMFNNLS, Vtall), streamed, snmf_snapshots]
if Vcsr is not None:
    cases.append(plain(pymf_amd.SNMF, Vcsr, compute_err=False))   # (no error on scipy.sparse data, as in the reference)
# 1. contexts created and closed over and over, every class, every kind of buffer (dense, CSR, streamed, snapshots)
_lib.load()
m0 = None
t_start = time.time()
for rep in range(60):
    for run in cases:
        mdl = run()
        if not np.all(np.isfinite(mdl.W)) or not np.all(np.isfinite(mdl.H)):
            bad += 1
        mdl._ctx.close(); mdl._ctx = None
    if rep == 4:
        m0, r0 = free_mib(), rss_mib()
m1, r1 = free_mib(), rss_mib()
print("contexts: %d in %.0f s" % (60 * len(cases), time.time() - t_start))
print("contexts: free device memory %.0f -> %.0f MiB, max RSS %.0f -> %.0f MiB" % (m0, m1, r0, r1))
if m0 - m1 > 64 or r1 - r0 > 256:
    bad += 1
# 2. one object, long free-running loops
mdl = pymf_amd.NMF(V, num_bases=16)
f0 = None
for rep in range(4):
    t0 = time.time()
    mdl.factorize(niter=20000, compute_err=(rep % 2 == 0))
    if rep == 0:
        f0, r0 = free_mib(), rss_mib()
    print("factorize(20000) %.2f s, len(ferr) %d, ferr[-1] %.6g" % (time.time() - t0, len(mdl.ferr) if hasattr(mdl, "ferr") and mdl.ferr is not None else 0,
                                                              mdl.ferr[-1] if rep % 2 == 0 else float("nan")), flush=True)
    if not np.all(np.isfinite(mdl.W)):
        bad += 1
f1, r1 = free_mib(), rss_mib()
print("long loops: free device memory %.0f -> %.0f MiB, max RSS %.0f -> %.0f MiB" % (f0, f1, r0, r1))
if f0 - f1 > 64 or r1 - r0 > 256:
    bad += 1
print("bad %d" % bad)
