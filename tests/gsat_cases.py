"""The cases of SIVM_GSAT (tests/test_gpu_gsat.py, tests/golden/gen_golden_gsat.py) and what makes the comparison with the
reference meaningful (tests/test_gsat_cases.py, no GPU).  Data are float32-representable and in general position, built as
sgreedy_cases.data builds its data (planted vertices among convex mixtures and noise); the walk starts from the first k columns
(init_w), which are mixtures, so the first batch already swaps several times.

name: (m, n, k, seed, niter, measure, start); seed feeds the data and np.random.seed before the walk.
  37 x 29, k = 5, 200 probes     fewer samples than a batch holds probes; many probes are skipped (in `select`)
  29 x 300, k = 6, 600 probes    odd row count; three batches, the last partial; l2 and l1
  70 x 200, k = 64, 400 probes   the widest LDS frame, every wave's work area
  5000 x 150, k = 8, 300 probes  the row loop of the distance step past one chunk (4096 rows); rows no multiple of 64
  16 x 120, k = 20, 100 probes   rows + 1 < k: every volume is rounding noise, in the reference too -- no golden, validity only

The reference itself can serve as the yardstick up to 19 bases only (REFERENCE_MAX_K).  vol.py:30-31 takes j = num_bases - 1
as a float32, and the factorial of a float32, its square and the product with 2^j stay float32: from 20 bases on the
denominator is inf, f1 = 0, every volume the reference computes is exactly 0, V stays 0, and every probe that is not in `select`
"wins" the tie and replaces vertex 0 (tests/test_gsat_cases.py evaluates the reference's expression to show it).  The device
folds the exact f1 into the pivots factor by factor in float64 and has real volumes at every width, so the 64-base case is held
against the float64 twin with the exact f1 (gsat_oracle.walk) with the same exactness as the goldens.

Below 20 bases the reference's f1 carries its float32 roundings: the gamma value, its square and the quotient, 2^-24 relative
each, 1.8e-07 on f1 at most and half of that on a volume (measured: 1.7e-09 .. 8.9e-08 on f1 at 9 .. 19 bases).  The twin with
reference_f1=True reproduces the goldens' _v to 1e-12; the device is held to 1e-10 against the twin with the exact f1 (float64
with another summation order) and to GOLDEN_V_TOL = 1e-07, the bound above, against the goldens themselves.
"""
import numpy as np

import gsat_oracle as go
import sgreedy_cases as sg

CASES = {
    "gsat_37x29_k5": (37, 29, 5, 31, 200, "l2", "init_w"),
    "gsat_29x300_k6_l2": (29, 300, 6, 32, 600, "l2", "init_w"),
    "gsat_29x300_k6_l1": (29, 300, 6, 33, 600, "l1", "init_w"),
    "gsat_70x200_k64": (70, 200, 64, 34, 400, "l2", "init_w"),
    "gsat_5000x150_k8": (5000, 150, 8, 35, 300, "l2", "init_w"),
}
DEGENERATE = {"gsat_16x120_k20": (16, 120, 20, 36, 100, "l2", "init_w")}
H_CASE = "gsat_29x300_k6_l2"          # factorize(niter=3) with H and ferr: golden gsat_29x300_k6_l2_h
REFERENCE_MAX_K = 19
TWIN_V_TOL = 1e-10
GOLDEN_V_TOL = 1e-7
GOLDEN_CASES = sorted(n for n, c in CASES.items() if c[2] <= REFERENCE_MAX_K)
TWIN_CASES = sorted(n for n, c in CASES.items() if c[2] > REFERENCE_MAX_K)
BATCH = 256
MIN_MARGIN = 1e-9
MIN_SWAPS = 5

_cache = {}


def data(name):
    """V float32 [m][n]"""
    if name not in _cache:
        m, n, k, seed, niter, measure, start = CASES.get(name) or DEGENERATE[name]
        _cache[name] = sg.data(m, n, k, seed, "wide" if k == 64 else None)[0]
    return _cache[name]


def spec(name):
    m, n, k, seed, niter, measure, start = CASES.get(name) or DEGENERATE[name]
    return dict(m=m, n=n, k=k, seed=seed, niter=niter, measure=measure, start=start)


def draws(name):
    s = spec(name)
    return go.draws(s["seed"], s["niter"], s["n"])


def twin(name, niter=None, reference_f1=False):
    """gsat_oracle.walk on the case: dict(idx, slots, select, W, v, V, margin), computed once"""
    key = (name, niter, reference_f1)
    if key not in _cache:
        s = spec(name)
        idx = draws(name)[:niter]
        r = go.walk(data(name).astype(np.float64), s["k"], idx, s["measure"], reference_f1=reference_f1)
        r["idx"] = idx
        _cache[key] = r
    return _cache[key]


def launches(slots, batch=BATCH):
    """Launch pairs the batch loop takes for these verdicts: one per batch and one more behind every accepted probe that
    is not the last of its batch"""
    count = 0
    for base in range(0, len(slots), batch):
        part = np.asarray(slots[base:base + batch])
        off = 0
        while off < len(part):
            count += 1
            acc = np.nonzero(part[off:] >= 0)[0]
            off = len(part) if len(acc) == 0 else off + int(acc[0]) + 1
    return count


def swaps_per_batch(slots, batch=BATCH):
    return [int((np.asarray(slots[b:b + batch]) >= 0).sum()) for b in range(0, len(slots), batch)]
