"""Planted problems for the non-negative QP kernels behind NMFALS / NMFNNLS (pmf_nnls.h, pmf_nnls_quad.h, pmf_nnls_wave.h):

    minimise 1/2 x' HA x - f' x   subject to x >= 0,      HA = H H^T (W half step) or W^T W (H half step).

A case fixes ONE half step and the X it starts from, and knows every problem's minimiser by construction: a passive set P,
x_P >= DX > 0 and multipliers lambda_N >= DL > 0 are chosen, f = HA x - lambda (lambda = 0 on P) satisfies the KKT conditions
with strict complementarity, and the data that produces this f is v = f' inv(HA) H (resp. W inv(HA) f), rounded to float32.
After the rounding the reference is RECOMPUTED from the float32 arrays in float64 (`f64`, then x_ref on P and w_ref on N), so
it is the exact minimiser of the problem the device is handed, not of the one that was planted.

The shared factor holds small dyadic numbers: HA = H H^T is then exact in float64 in any summation order (the device forms it
in float64), and S = W^T W of the H half step is exact in the float32 the device forms it in (k_hessian_from_ps reads it).

Bounds, from the reference alone (nothing here is measured on a device):
    eps_f   = len 2^-23 (|V| |H|^T)          worst case of a float32 product of `len` terms in any summation order (the fp32 MFMA
                                             does not round its running sum to nearest: DESIGN.md section 4), per entry of f
    bound_x = ||inv(HA[P,P])||_inf max_P eps_f + 2^-24 |x_ref|        (the solve in float64, the result stored as float32)
    bound_w = max eps_f (1 + ||HA[N,P] inv(HA[P,P])||_inf)
The cases are well-posed when min x_ref[P] > 2 bound_x and min -w_ref[N] > 2 bound_w: then every solver that is right to its
bound finds exactly the support P.  tests/test_nnqp_cases.py checks that on the CPU; tests/test_gpu_nnqp_cases.py runs the
device kernels against it."""
import functools
from math import gcd

import numpy as np

EPS32 = 2.0 ** -23
QUAD_K = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
WAVE_K = (65, 96, 127, 128)
BIG_K = (100, 129, 256, 257)          # k_nnqp_big with 2 (nnqp_wave = 0), 4, 4 and 8 variables per lane (16 per lane, k > 512: not covered)
STARTS = ("zeros", "ones", "support", "complement", "random")
# where the passive variables sit; cycled per problem (period 5: coprime to the 4 problems of a wave and the 48 of a
# 12-wave workgroup, and to the length of every size list below, so every size meets every position)
POSITIONS = ("random", "lowest", "highest", "per16", "random")
FLAG_MIN_PIVOT = 1e-8                 # k_inverse_spd_mfma's `spd_flag` / k_spd_unique_big: smallest pivot ratio that keeps the fast kernels


def quad_sizes(k):
    """|P| at which min(|P|, k - |P|) crosses 16 | 17 (the frame boundary) from both sides, and the primal / complement switch."""
    c = (0, 1, 15, 16, 17, k // 2 - 1, k // 2, k // 2 + 1, k - 17, k - 16, k - 15, k - 1, k)
    return sorted(set(p for p in c if 0 <= p <= k))


def lane_sizes(k):
    return sorted(set(p for p in (0, 1, k // 2, k - 1, k) if 0 <= p <= k))


def wave_sizes(k):
    return sorted(set(p for p in (0, 1, 63, 64, 65, k - 64, k - 1, k) if 0 <= p <= k))


def size_cycle(sizes):
    """The sizes, the first ones repeated until the length is coprime to 2, 3 and 5 (a wave's 4 problems, a workgroup's 48 and
    the 5 positions): neighbouring problems differ in size, and a deferred problem sits beside solved ones."""
    out = list(sizes)
    i = 0
    while gcd(len(out), 30) != 1:
        out.append(sizes[i % len(sizes)])
        i += 1
    return out


def place(rule, live, p, rng):
    """p passive variables among the live ones.  per16: one per block of 16 first -- in k_nnqp_quad variable 16 s + r is slot s of
    lane r, so this fills lane 0's slots, then lane 1's; in k_nnqp_wave it alternates between a lane's two variables."""
    if rule == "lowest":
        return live[:p]
    if rule == "highest":
        return live[len(live) - p:]
    if rule == "per16":
        order = sorted(live, key=lambda v: (v % 16, v // 16))
        return np.sort(np.asarray(order[:p], dtype=np.int64))
    return np.sort(rng.choice(live, size=p, replace=False))


def min_pivot_ratio(HA):
    """Smallest pivot of the unpivoted LDL^T of HA scaled to a unit diagonal, dead (zero) variables left out: what the device's
    flag compares with 1e-8."""
    d = np.diag(HA)
    live = np.flatnonzero(d > 1e-12 * d.max())
    s = 1.0 / np.sqrt(d[live])
    A = HA[np.ix_(live, live)] * s[:, None] * s[None, :]
    piv = []
    for j in range(A.shape[0]):
        piv.append(A[j, j])
        if not A[j, j] > 0:
            return min(piv)
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:]) / A[j, j]
    return min(piv)


def int_factor(rng, k, ln, amp):
    """k x ln, integers in [-amp, amp]: full row rank (checked by the CPU test through the pivots), HA exact."""
    return rng.randint(-amp, amp + 1, size=(k, ln)).astype(np.float32)


class Case(object):
    """One half step.  step 'w': problems are the rows of V (nprob x ln), factor = H (k x ln).  step 'h': problems are the
    columns of V (ln x nprob), factor = W (ln x k) -- `factor` is stored k x ln either way, `V` problem-major (nprob x ln).
    P: bool (nprob x k).  X0: float32 (nprob x k).  x_ref, w_ref, f64, eps_f: float64 (nprob x k).  bound_x, bound_w: (nprob,)."""

    def __init__(self, name, step, factor, P, start, seed, x_lo=1.0, lam_rel=0.25, tie=None):
        rng = np.random.RandomState(seed)
        self.name, self.step, self.start = name, step, start
        self.factor = np.ascontiguousarray(factor, dtype=np.float32)
        self.k, self.ln = self.factor.shape
        self.P = P
        self.nprob = P.shape[0]
        F = self.factor.astype(np.float64)
        self.HA = HA = F.dot(F.T)
        d = np.diag(HA)
        self.live = live = d > 1e-12 * d.max()
        assert not P[:, ~live].any()
        HAp = HA.copy()
        HAp[~live, :] = 0.0
        HAp[:, ~live] = 0.0
        HAp[~live, ~live] = 1.0
        # ---- plant: x on P, lambda on the live rest, f = HA x - lambda, data = f' inv(HA) factor ----
        x = np.where(P, x_lo * (1.0 + rng.random_sample(P.shape)), 0.0)
        lam = np.where(~P & live[None, :], lam_rel * d[live].mean() * (1.0 + rng.random_sample(P.shape)), 0.0)
        if tie is not None:
            lam[:, tie[1]] = lam[:, tie[0]]
        f = x.dot(HA) - lam
        self.V = np.ascontiguousarray(np.linalg.solve(HAp, f.T).T.dot(F), dtype=np.float32)
        # ---- recompute the reference from the float32 arrays ----
        V64 = self.V.astype(np.float64)
        self.f64 = V64.dot(F.T)
        self.eps_f = self.ln * EPS32 * np.abs(V64).dot(np.abs(F.T))
        self.x_ref = np.zeros_like(f)
        self.w_ref = np.zeros_like(f)
        self.bound_x = np.zeros(self.nprob)
        self.bound_w = np.zeros(self.nprob)
        for i in range(self.nprob):
            p = np.flatnonzero(P[i])
            nn = np.flatnonzero(~P[i] & live)
            ef = self.eps_f[i, live].max()
            if p.size:
                inv = np.linalg.inv(HA[np.ix_(p, p)])
                self.x_ref[i, p] = np.linalg.solve(HA[np.ix_(p, p)], self.f64[i, p])
                self.w_ref[i, nn] = self.f64[i, nn] - HA[np.ix_(nn, p)].dot(self.x_ref[i, p])
                self.bound_x[i] = np.abs(inv).sum(axis=1).max() * self.eps_f[i, p].max()
                cross = np.abs(HA[np.ix_(nn, p)].dot(inv)).sum(axis=1).max() if nn.size else 0.0
                self.bound_w[i] = ef * (1.0 + cross)
            else:
                self.w_ref[i, nn] = self.f64[i, nn]
                self.bound_w[i] = ef
        # ---- the X the half step starts from (its support seeds the passive set; the minimiser does not depend on it) ----
        if start == "zeros":
            X0 = np.zeros(P.shape)
        elif start == "ones":
            X0 = np.ones(P.shape)             # (a dead variable too: the kernels must keep it out)
        elif start == "support":
            X0 = P.astype(np.float64)
        elif start == "complement":
            X0 = (~P).astype(np.float64)
        else:
            X0 = (rng.random_sample(P.shape) < 0.5).astype(np.float64)
        self.X0 = np.ascontiguousarray(X0, dtype=np.float32)

    def bound_x_elem(self):
        """|x_dev - x_ref| <= this, elementwise (zero off the support: those entries must be exactly 0)."""
        return self.bound_x[:, None] * self.P + 2.0 ** -24 * np.abs(self.x_ref)

    def sys_size(self):
        """s = min(|P|, klive - |P|): the system a problem factorises in k_nnqp_quad / k_nnqp_wave."""
        np_ = self.P.sum(axis=1)
        return np.minimum(np_, int(self.live.sum()) - np_)


def supports(sizes, nprob, live, k, rng):
    P = np.zeros((nprob, k), dtype=bool)
    cyc = size_cycle(sizes)
    for i in range(nprob):
        P[i, place(POSITIONS[i % len(POSITIONS)], live, cyc[i % len(cyc)], rng)] = True
    return P


def contraction(k):
    return 128 if k <= 64 else 320 if k <= 128 else 640


def _seed(*parts):
    return int(sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31 - 1))


# ---- the catalogue: name -> (builder arguments); built on demand, once ---------------------------------------------------------
# kind: which size list; step; k; start; nprob.  The GPU file decides the options (which kernel runs) per kind.
SPECS = {}


def _add(name, **kw):
    assert name not in SPECS
    SPECS[name] = kw


for _k in QUAD_K:                                   # k_nnqp_quad (nnqp_quad = 2, both frames) and k_nnqp (nnqp_quad = 0)
    for _s in STARTS:
        _add("w_k%d_%s" % (_k, _s), kind="quad", step="w", k=_k, start=_s, nprob=203)
for _k in WAVE_K:                                   # k_nnqp_wave
    for _s in STARTS:
        _add("w_k%d_%s" % (_k, _s), kind="wave", step="w", k=_k, start=_s, nprob=131)
for _k in BIG_K:                                    # k_nnqp_big (at 100 bases: nnqp_wave = 0); slow: 67 problems
    for _s in STARTS:
        _add("wbig_k%d_%s" % (_k, _s), kind="big", step="w", k=_k, start=_s, nprob=67)
for _k in (17, 48, 64):                             # H half step (problem = column): the frame-boundary sizes
    for _s in ("zeros", "support", "random"):
        _add("h_k%d_%s" % (_k, _s), kind="quad", step="h", k=_k, start=_s, nprob=203)
for _k in (96, 128):
    for _s in ("zeros", "support", "random"):
        _add("h_k%d_%s" % (_k, _s), kind="wave", step="h", k=_k, start=_s, nprob=131)
_add("w_k48_dead", kind="quad", step="w", k=48, start="ones", nprob=203, dead=5)        # H row 5 is zero: a dead basis
# grid stride: one partial sweep beyond the grid caps (512 workgroups x 16 problems; 256 x 48), and the default switch
_add("w_k48_grid32", kind="quad", step="w", k=48, start="random", nprob=8192 + 16 + 3)
# (grid16 starts from the exact support: a random 50 % support at k = 48 has min(|P0|, 48 - |P0|) > 16 for 97 % of the problems, which
# the 16-slot frame hands on in pass 0 without a solve -- the planted sizes must stay in the frame for it to stride with work)
_add("w_k48_grid16", kind="quad", step="w", k=48, start="support", nprob=12288 + 48 + 3)
_add("w_k64_default", kind="quad", step="w", k=64, start="random", nprob=16384 + 5)
LADDER = {"1e-3": (1, 5), "1e-5": (13, 12), "1e-7": (83, 18)}      # rung: row j = row i + (a 2^-b) e
for _k in (32, 64):
    for _r in LADDER:
        _add("ladder_k%d_%s" % (_k, _r), kind="ladder", step="w", k=_k, start="zeros", nprob=203, rung=_r)

QUAD_W = [n for n, s in SPECS.items() if s["kind"] == "quad" and s["step"] == "w"]
QUAD_H = [n for n, s in SPECS.items() if s["kind"] == "quad" and s["step"] == "h"]
WAVE = [n for n, s in SPECS.items() if s["kind"] == "wave"]
BIG = [n for n, s in SPECS.items() if s["kind"] == "big"]
LADDERS = [n for n, s in SPECS.items() if s["kind"] == "ladder"]
LADDER_PAIR = (3, 7)                  # the nearly collinear rows of the ladder's H


def sizes_of(spec):
    k = spec["k"] - (1 if "dead" in spec else 0)
    return {"quad": quad_sizes, "ladder": lane_sizes, "wave": wave_sizes, "big": lane_sizes}[spec["kind"]](k)


@functools.lru_cache(maxsize=None)
def case(name):
    spec = SPECS[name]
    k, nprob, step = spec["k"], spec["nprob"], spec["step"]
    seed = _seed(k, nprob, STARTS.index(spec["start"]), len(name))
    rng = np.random.RandomState(seed)
    ln = contraction(k) if step == "w" else max(2 * k, 64)
    # W of the H half step: |entries| <= 3, so S = W^T W (sums of at most 256 products <= 9) is exact in float32
    fac = int_factor(rng, k, ln, 4 if step == "w" else 3)
    live = np.arange(k)
    if "dead" in spec:
        fac[spec["dead"], :] = 0.0
        live = np.delete(live, spec["dead"])
    if spec["kind"] == "ladder":
        # rows i, j nearly collinear: the last pivot ratio of the pair is about (a 2^-b)^2 |e_perp|^2 / |row j|^2.  What the
        # margins of a float32 right-hand side (eps_f ~ len 2^-23 |V| |H|) leave room for, worked out on the host:
        #  * both rows passive: ||inv(HA[P,P])||_inf ~ 1 / (ratio |row|^2), bound_x = 0.7 at x = 1 already at the 1e-3 rung;
        #  * one passive, one not: w_j = w_i + O(a 2^-b) = O(a 2^-b), no multiplier of size DL fits (planting one puts
        #    lambda_j / (a 2^-b |e|) into V and eps_f with it: margin 1.2 instead of 2 at the 1e-7 rung).
        # So at the minimiser both rows are at zero with EQUAL multipliers, and the final HA[P,P] is well conditioned.  What the
        # rung still reaches: from the zeros start the first exchange takes in every variable with f > tol, the pair among them
        # in 10 of 203 problems at k = 32 and 42 - 45 of 203 at k = 64 (pair_enters_first below; the CPU test holds the counts
        # above zero), so those problems factorise an ill-conditioned HA[P,P] on the way; and B = inv(HA), blocks of which the
        # complement form factorises, is ill-conditioned for every problem.
        a, b = LADDER[spec["rung"]]
        i, j = LADDER_PAIR
        e = rng.randint(-4, 5, size=ln)
        fac[j, :] = fac[i, :] + np.float32(a * 2.0 ** -b) * e.astype(np.float32)
        P = np.zeros((nprob, k), dtype=bool)
        for q in range(nprob):
            P[q, rng.choice(k, size=rng.randint(0, k + 1), replace=False)] = True
            P[q, i] = P[q, j] = False
    else:
        P = supports(sizes_of(spec), nprob, live, k, rng)
    return Case(name, step, fac, P, spec["start"], seed + 1, tie=LADDER_PAIR if spec["kind"] == "ladder" else None)


def pair_enters_first(c):
    """Problems of a ladder case whose nearly collinear pair becomes passive TOGETHER in the first exchange from the zeros start
    (w = f there; the kernels' entering rule is w > tol = eps k max diag HA)."""
    i, j = LADDER_PAIR
    tol = 2.220446049250313e-15 * c.k * np.diag(c.HA).max()
    return np.flatnonzero((c.f64[:, i] > tol) & (c.f64[:, j] > tol))


# ---- the frame sequence: four W half steps of ONE context at k = 48, exact-support start ---------------------------------------
SEQ_K, SEQ_NPROB = 48, 1001
SEQ_SHARES = (0.0, 0.05, 0.5, 0.0)   # share of problems with s > 16 (steps 2, 3: s in 17 .. 24)


@functools.lru_cache(maxsize=None)
def sequence():
    rng = np.random.RandomState(4801)
    fac = int_factor(rng, SEQ_K, contraction(SEQ_K), 4)
    live = np.arange(SEQ_K)
    out = []
    for step, share in enumerate(SEQ_SHARES):
        nbig = int(round(share * SEQ_NPROB))
        big = np.zeros(SEQ_NPROB, dtype=bool)
        big[rng.choice(SEQ_NPROB, size=nbig, replace=False)] = True
        P = np.zeros((SEQ_NPROB, SEQ_K), dtype=bool)
        for q in range(SEQ_NPROB):
            s = rng.randint(17, 25) if big[q] else rng.randint(0, 17)
            p = s if rng.randint(2) else SEQ_K - s
            P[q, place(POSITIONS[q % 5], live, p, rng)] = True
        out.append(Case("seq_step%d" % (step + 1), "w", fac, P, "support", 4802 + step))
    return out


# ---- the fallback: HA singular (a duplicated row), flag 0, the kernels fall back on the device -----------------------------------
@functools.lru_cache(maxsize=None)
def fallback(k):
    """k = 24 (k_nnqp_quad -> k_nnqp) or 100 (k_nnqp_wave -> k_nnqp_big): H row 7 = row 3.  Not planted: the minimiser is not
    unique, the checks are KKT and the objective.  Returns H, V (float32) and f64, eps_f, HA (float64)."""
    rng = np.random.RandomState(700 + k)
    ln, nprob = contraction(k), (203 if k <= 64 else 67)
    H = int_factor(rng, k, ln, 4)
    H[7, :] = H[3, :]
    x = np.where(rng.random_sample((nprob, k)) < 0.4, 1.0 + rng.random_sample((nprob, k)), 0.0)
    V = np.ascontiguousarray(x.dot(H.astype(np.float64)) + 8.0 * rng.standard_normal((nprob, ln)), dtype=np.float32)
    H64, V64 = H.astype(np.float64), V.astype(np.float64)
    return dict(H=H, V=V, HA=H64.dot(H64.T), f64=V64.dot(H64.T), eps_f=ln * EPS32 * np.abs(V64).dot(np.abs(H64.T)), k=k, ln=ln, nprob=nprob)
