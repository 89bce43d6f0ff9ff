"""The device cases of AA (tests/test_gpu_aa.py) and what makes the comparison with the float64 oracle meaningful
(tests/test_aa_cases.py, no GPU): the smallest shapes at which the kernels can go wrong.

Data are the planted mixtures of tests/sivm_cases.py (float32-representable).  H0 is the reference's init_h (uniform, columns
normalised) rounded to float32, so that the device and the oracle start from the same numbers; W_hat = V pinv(H0) then lies
far outside the hull and every base ends on a face of it.  'dup' repeats data columns (pricing ties, a corral that must not
take the twin); 'inside' chooses H0 = pinv(beta0^T) for strictly positive convex weights beta0, so that W_hat = V beta0^T lies
strictly inside the hull: the projection is W_hat itself.
"""
import numpy as np

import aa_oracle as ao
import sivm_cases as sc

# name: (m, n, k, seed, special)
CASES = {
    "37x29_k5": (37, 29, 5, 31, None),             # odd m, n under one panel, n < m: beta is unique
    "29x300_k6": (29, 300, 6, 32, None),           # ragged last panel, n > m: beta is not unique
    "64x4096_k64": (64, 4096, 64, 33, None),       # full width in k and m
    "8x70000_k3": (8, 70000, 3, 34, None),         # more than 1024 panels: a workgroup owns several; k below one MFMA tile
    "300x128_k5": (300, 128, 5, 37, None),         # taller than the 128 rows of R staged at a time; 128 columns: the largest corral frame
    "16x200_k4_dup": (16, 200, 4, 35, "dup"),
    "12x200_k4_inside": (12, 200, 4, 36, "inside"),
}

# Worst deviation, over all cases, between the all-float64 oracle (exact projection, exact H step) and the restated device
# rounds with W_hat from a float32 product (aa_oracle.w_hat_f32), float32 V, R, X and g, followed by the H step with float32 W, right-hand sides and X
# (tests/test_aa_cases.py re-measures them per case and holds them to these figures); the tolerances of the device comparison
# are 4 x the worst, the margin SIVM's H_TOL and FERR_TOL use.
#   W (relative Frobenius): 5.76e-07 at 8x70000_k3 (W_hat lies inside the hull there: the rounds stop at a residual of 1e-6;
#                           4.93e-07 at 12x200_k4_inside, 4.09e-07 at 64x4096_k64, 5.6e-08 .. 6.3e-08 everywhere else)
#   H (relative Frobenius): 9.69e-05 at 8x70000_k3 (cond(W^T W) = 1e6; 3.88e-05 at 12x200_k4_inside, below 1e-06 elsewhere)
#   ferr (relative):        1.84e-08 at 16x200_k4_dup (1.52e-08 at 8x70000_k3, below 8e-09 everywhere else)
MEASURED_W = 5.76e-07
MEASURED_H = 9.69e-05
MEASURED_FERR = 1.84e-08
W_TOL = 4.0 * MEASURED_W
H_TOL = 4.0 * MEASURED_H
FERR_TOL = 4.0 * MEASURED_FERR

ROUND_CAP = 512          # PMF_AA_ROUND_CAP (pymf_amd/csrc/pmf_host_aa.h)
MIN_RANK_MARGIN = 1e-3   # smallest singular value of H0 over the largest
MAX_CORRAL = ao.AA_MAX_CORRAL

_cache = {}


def data(name):
    """(V float32, k, H0 float64 holding float32 values, W0)."""
    m, n, k, seed, special = CASES[name]
    V, _ = sc.planted(m, n, k, seed)
    rng = np.random.RandomState(seed + 1000)
    if special == "dup":
        V[:, 5] = V[:, 150]
        V[:, 6] = V[:, 150]
        V[:, 90] = V[:, 17]
    H0 = rng.random_sample((k, n))
    H0 /= H0.sum(axis=0)
    if special == "inside":
        beta0 = 0.5 * rng.dirichlet(np.full(n, 0.5), size=k) + 0.5 / n
        H0 = np.linalg.pinv(beta0.T)
    H0 = ao.f32(H0)
    W0 = rng.random_sample((m, k))
    return V, k, H0, W0


def case(name):
    """dict(V, k, H0, W0, Wh, W, beta, H, ferr): one iteration of the float64 oracle on the float32-representable data."""
    if name in _cache:
        return _cache[name]
    V, k, H0, W0 = data(name)
    V64 = V.astype(np.float64)
    W, beta, Wh = ao.update_w(V64, H0)
    H, ferr = ao.update_h(V64, W)
    _cache[name] = dict(V=V, k=k, H0=H0, W0=W0, Wh=Wh, W=W, beta=beta, H=H, ferr=ferr, special=CASES[name][4])
    return _cache[name]
