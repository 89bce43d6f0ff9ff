"""CNMF cases beyond tests/test_gpu_cnmf.py: every width of k_cnmf_mul_step (NT = 1, 2, 4, 8) at its lowest and highest k,
ragged k and n, mixed-sign data at every width, tiny m and n, the multi-row-block chunks of the dense V^T V, and the paths of
the host loop (chunk boundaries, the stop state 2 of k_conv_check, loops without the error or without the G step).  Data,
start states and float64 oracle runs (tests/cnmf_oracle.py), and the same runs with C formed in float32 and W rounded to
float32 ("f32": what the float32 data path alone costs) -- each computed once and shared by tests/test_cnmf_cases.py (no GPU:
the cases leave room for float32) and tests/test_gpu_cnmf_cases.py."""
import collections
import functools
import random

import numpy as np

import cnmf_oracle as co

Case = collections.namedtuple("Case", "m n k seed noise shift")
SEED = 7


def planted(m, n, k, rseed, noise=0.05, shift=0.0):
    """Data with k well separated clusters of samples whose first members are exactly the samples random.sample draws
    under random.seed(rseed): the k-means has no near-ties to decide.  shift = 0.5: centres and noise are centred on zero,
    so about half of C = V^T V is negative."""
    random.seed(rseed)
    sel = np.sort(random.sample(range(n), k))
    labels = np.arange(n) % k
    rest = np.setdiff1d(np.arange(n), sel)
    labels[sel] = np.arange(k)
    labels[rest] = np.arange(len(rest)) % k
    rs = np.random.RandomState(rseed)
    centres = rs.random_sample((m, k)) - shift
    V = centres[:, labels] + noise * (rs.random_sample((m, n)) - (0.5 if shift else 0.0))
    return V.astype(np.float32), sel, labels


# (m, n, k): what the shape is meant for (tests/test_cnmf_cases.py derives it from the formulas of pmf_create / ensure_vgram)
WIDTH_SHAPES = [
    (70, 64, 16),       # NT 1 full, np = 64: one k-step round of k_cnmf_split_gemm
    (70, 65, 17),       # NT 2 at its smallest, np = 128 with 63 padded columns
    (33, 130, 32),      # NT 2 full
    (70, 200, 33),      # NT 4 at its smallest
    (129, 192, 64),     # NT 4 full, n a multiple of 64
    (70, 130, 65),      # NT 8 at its smallest
    (70, 200, 100),     # NT 8 ragged
    (300, 128, 128),    # NT 8 full, n == k
    (70, 70, 47),       # NT 4 ragged
    (5, 64, 3),         # m < 16
    (70, 17, 17),       # n == k, n barely above 16: every cluster has one member
    (8245, 64, 6),      # ensure_vgram: 516 row blocks of 16, rpc = 32
]
SHIFTS = (0.0, 0.5)
WIDTH_CASES = [Case(m, n, k, SEED, 0.05, s) for (m, n, k) in WIDTH_SHAPES for s in SHIFTS]
WIDTH_NITER = (8, 40)

# one iteration from a dense random start, one shape per NT: H only, G only, both
ONE_STEP_CASES = [Case(m, n, k, SEED, 0.05, 0.5) for (m, n, k) in [(70, 64, 16), (70, 65, 17), (70, 200, 33), (70, 200, 100)]]
ONE_STEP_MODES = [("H", False, True), ("G", True, False), ("GH", True, True)]          # (name, compute_w, compute_h)

# the host loop: the free-running loop starts after iteration 0 when two iterations are left, in chunks of 32
LOOP_CASE = Case(40, 64, 4, SEED, 0.05, 0.0)
LOOP_NITER = (1, 2, 3, 33, 34, 70)
CHUNK = 32
NO_ERR_NITER = 5
NO_G_NITER = (5, 40)
TWICE_NITER = 35           # the second call starts below 1e-2 tr(C): all of it runs iteration by iteration
TWICE_EARLY_NITER = 8      # the second call starts above it: chunks again, with dStop and dFerr left over from the first

# e^2 / tr(C) starts above 1e-2 and falls below 1e-3 in the middle of the second chunk: stop state 2 of k_conv_check
CANCEL_CASE = Case(40, 64, 2, SEED, 0.001, 0.0)
CANCEL_NITER = 70

# the k-means initialisation; (70, 17, 17) and (70, 20, 17) have clusters of exactly one member
INIT_SHAPES = [(70, 65, 17), (70, 200, 33), (70, 200, 100), (70, 17, 17), (70, 20, 17), (5, 64, 3)]
INIT_CASES = [Case(m, n, k, SEED, 0.05, s) for (m, n, k) in INIT_SHAPES for s in SHIFTS]
ONE_MEMBER_SHAPES = [(70, 17, 17), (70, 20, 17)]

PLANTED_CASES = list(dict.fromkeys(WIDTH_CASES + ONE_STEP_CASES + [LOOP_CASE, CANCEL_CASE] + INIT_CASES))


def case_id(c):
    return "%dx%d-k%d-noise%g-shift%g" % (c.m, c.n, c.k, c.noise, c.shift)


def r32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def data(c):
    """(V float32, sel, labels)"""
    return frozen(*planted(c.m, c.n, c.k, c.seed, c.noise, c.shift))


@functools.lru_cache(maxsize=None)
def start(c):
    """The reference's initialisation in float64 -> (H0, G0, assigned, smallest relative distance gap of the k-means)."""
    V, sel, _ = data(c)
    Vd = V.astype(np.float64)
    H0, G0, assigned = co.cnmf_init(Vd, c.k, sel)
    return frozen(H0, G0, assigned) + (co.kmeans(Vd, c.k, sel)[2],)


@functools.lru_cache(maxsize=None)
def dense_start(c):
    """(H0, G0): dense random float64 factors, not the near-one-hot k-means start."""
    rs = np.random.RandomState(11)
    return frozen(rs.random_sample((c.k, c.n)), rs.random_sample((c.n, c.k)) / 3.0)


def gram32(c):
    """C as float32 arithmetic on the float32 data forms it."""
    V = data(c)[0]
    return V.T.dot(V).astype(np.float64)


@functools.lru_cache(maxsize=None)
def oracle(c, niter, compute_w=True, compute_h=True, compute_err=True, dense=False, f32=False, calls=1):
    """`calls` factorize(niter) calls in a row from start(c) (dense: dense_start(c)) -> (W, H, G, ferr) of the last one."""
    V = data(c)[0].astype(np.float64)
    H, G = dense_start(c) if dense else start(c)[:2]
    kw = dict(gram=gram32(c), w_round=r32) if f32 else {}
    for _ in range(calls):
        W, H, G, ferr = co.cnmf_factorize(V, H, G, niter=niter, compute_w=compute_w, compute_h=compute_h,
                                          compute_err=compute_err, **kw)
    return frozen(W, H, G, ferr)


# ---- the runs: (case, arguments of factorize) ----------------------------------------------------------------------------
Run = collections.namedtuple("Run", "c niter compute_w compute_h compute_err dense calls")


def run(c, niter, compute_w=True, compute_h=True, compute_err=True, dense=False, calls=1):
    return Run(c, niter, compute_w, compute_h, compute_err, dense, calls)


def run_id(r):
    return "%s-niter%d%s%s%s%s%s" % (case_id(r.c), r.niter, "" if r.compute_w else "-noG", "" if r.compute_h else "-noH",
                                     "" if r.compute_err else "-noerr", "-dense" if r.dense else "",
                                     "-x%d" % r.calls if r.calls > 1 else "")


def run_oracle(r, f32=False):
    return oracle(r.c, r.niter, r.compute_w, r.compute_h, r.compute_err, r.dense, f32, r.calls)


WIDTH_RUNS = [run(c, niter) for c in WIDTH_CASES for niter in WIDTH_NITER]
ONE_STEP_RUNS = [run(c, 1, cw, ch, dense=True) for c in ONE_STEP_CASES for (_, cw, ch) in ONE_STEP_MODES]
LOOP_RUNS = [run(LOOP_CASE, niter) for niter in LOOP_NITER]
NO_ERR_RUN = run(LOOP_CASE, NO_ERR_NITER, compute_err=False)
NO_G_RUNS = [run(LOOP_CASE, niter, compute_w=False) for niter in NO_G_NITER]
TWICE_RUN = run(LOOP_CASE, TWICE_NITER, calls=2)
TWICE_EARLY_RUN = run(LOOP_CASE, TWICE_EARLY_NITER, calls=2)
CANCEL_RUN = run(CANCEL_CASE, CANCEL_NITER)
ALL_RUNS = WIDTH_RUNS + ONE_STEP_RUNS + LOOP_RUNS + [NO_ERR_RUN] + NO_G_RUNS + [TWICE_RUN, TWICE_EARLY_RUN, CANCEL_RUN]


# `data` replaced under a live object by data of another sign pattern: C, its trace, A, B and L are all formed again
REPLACE_FROM, REPLACE_TO, REPLACE_NITER = Case(70, 65, 17, SEED, 0.05, 0.0), Case(70, 65, 17, SEED, 0.05, 0.5), 8


@functools.lru_cache(maxsize=None)
def replaced_oracle(f32=False):
    """factorize(8) on REPLACE_FROM, then factorize(8) from its H and G on the data of REPLACE_TO -> (W, H, G, ferr)."""
    _, H, G, _ = oracle(REPLACE_FROM, REPLACE_NITER, f32=f32)
    kw = dict(gram=gram32(REPLACE_TO), w_round=r32) if f32 else {}
    return frozen(*co.cnmf_factorize(data(REPLACE_TO)[0].astype(np.float64), H, G, niter=REPLACE_NITER, **kw))


def trace(c):
    V = data(c)[0].astype(np.float64)
    return float(np.sum(V * V))


def geometry(m, n, k):
    """What pmf_create and ensure_vgram (dense data) derive from a shape."""
    NT = 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8
    KP, np_, mp = 16 * NT, -(-n // 64) * 64, -(-m // 64) * 64
    blocks16 = mp // 16
    gchunks = min(512, blocks16)
    rpc = -(-blocks16 // gchunks) * 16
    return dict(NT=NT, KP=KP, np=np_, rounds=np_ // 64, pad_rows=KP - k, pad_cols=np_ - n, blocks16=blocks16, rpc=rpc,
                gchunks=-(-mp // rpc))
