"""The non-negative QP kernels of NMFALS (k_nnqp, k_nnqp_quad on both frames, k_nnqp_wave, k_nnqp_big and their device-side
fallback) on the MI355X against the planted problems of tests/nnqp_cases.py: ONE half step per case through the C ABI, every
problem compared on its own -- support exactly the planted one, |x_dev - x_ref| <= bound_x elementwise (the bound comes from
the float64 reference, tests/nnqp_cases.py; tests/test_nnqp_cases.py shows on the CPU that it leaves the support determined).
The worst |x_dev - x_ref| / bound_x of every run goes to parity_nnqp.json beside the session's ledger (committed as
profiles/parity_nnqp.json); a ratio above 1 fails, and no other tolerance appears in the planted tests.  The fallback test,
whose minimiser is not unique, compares against bounds derived the same way and carries two float64 slack literals (1e-12 of
max |f| on the dual, 1e-9 relative on the objective: the accuracy of the float64 oracle it is compared with)."""
import json
import os

import numpy as np
import pytest

import nnqp_cases as nc
from conftest import LEDGER_PATH
from oracle.nmfals_oracle import nnqp_solve
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

_parity = {}
_fallback = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    try:
        out = os.path.dirname(LEDGER_PATH)                    # beside the session's ledger; committed as profiles/parity_nnqp.json
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_nnqp.json"), "w") as f:
            json.dump({"worst |x_dev - x_ref| / bound_x": _parity, "fallback: worst objective gap / bound": _fallback}, f, indent=1,
                      sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def _context(c, opts):
    m, n = (c.nprob, c.ln) if c.step == "w" else (c.ln, c.nprob)
    ctx = _lib.Context(_lib.ALGO_NMFALS, m, n, c.k)
    for name, value in opts.items():
        ctx.set_option(name, value)
    return ctx


def _half_step(ctx, c, V=None, X0=None):
    """Upload and run the one half step of the case; the result problem-major (nprob x k)."""
    V = c.V if V is None else V
    X0 = c.X0 if X0 is None else X0
    if c.step == "w":
        ctx.set_v_dense(V)
        ctx.set_w(X0)
        ctx.set_h(c.factor)
        ctx.update_w()
        return ctx.get_w()
    ctx.set_v_dense(np.ascontiguousarray(V.T))
    ctx.set_w(np.ascontiguousarray(c.factor.T))
    ctx.set_h(np.ascontiguousarray(X0.T))
    ctx.update_h()
    return np.ascontiguousarray(ctx.get_h().T)


def _prime(ctx, c):
    """A half step of the same kind on zero data (f = 0: every problem ends at once with an empty passive set) leaves the
    history 'no problem beyond 16 unknowns' -- the next one runs the 16-slot frame with the 32-slot frame behind it."""
    out = _half_step(ctx, c, V=np.zeros_like(c.V), X0=np.zeros_like(c.X0))
    assert not out.any()


def _check(c, x_dev, run):
    x_dev = np.asarray(x_dev, dtype=np.float64)
    assert x_dev.shape == c.x_ref.shape
    assert np.isfinite(x_dev).all() and (x_dev >= 0).all(), run
    wrong = np.flatnonzero(((x_dev > 0) != c.P).any(axis=1))
    err = np.abs(x_dev - c.x_ref)
    bound = c.bound_x_elem()
    ratio = float(np.where(c.P, err / np.where(c.P, bound, 1.0), 0.0).max()) if c.P.any() else 0.0
    print("%-40s worst |x_dev - x_ref| / bound_x = %.3e, wrong supports: %d of %d" % (run, ratio, wrong.size, c.nprob))
    _parity[run] = ratio
    assert wrong.size == 0, (run, "support differs from the planted one at problems", wrong[:8].tolist(),
                             "sizes", c.P[wrong[:8]].sum(axis=1).tolist())
    assert (x_dev[:, ~c.live] == 0).all(), (run, "a dead basis left zero")
    assert (err <= bound).all(), (run, ratio)


def _run(name, opts, prime=False, tag=""):
    """-> k_nnqp_quad's counters of the half step under test (all zero unless opts holds nnqp_count = 1 on a W half step)."""
    c = nc.case(name)
    ctx = _context(c, opts)
    try:
        if prime:
            _prime(ctx, c)
            ctx.nnqp_counters(reset=True)
        x = _half_step(ctx, c)
        cnt = ctx.nnqp_counters(reset=True)
    finally:
        ctx.close()
    _check(c, x, name + tag)
    return cnt


def _assert_split(c, cnt, run):
    """Exact-support start: the first solve of a problem is its last and a problem beyond the frame is listed before any
    solve, so the 16-slot frame solves exactly the problems with s <= 16 and the 32-slot frame exactly the rest."""
    nbig = int((c.sys_size() > 16).sum())
    s16, s32 = cnt["frame16"]["problems"], cnt["frame32"]["problems"]
    print("%-40s solved16 = %d, solved32 = %d, planted s > 16: %d of %d" % (run, s16, s32, nbig, c.nprob))
    assert cnt["frame16"]["wave_tasks"] > 0, (run, "the 16-slot frame did not run", cnt)
    assert s16 == c.nprob - nbig and s32 == nbig, (run, cnt)


# ---- k_nnqp_quad: the 32-slot frame alone, and the 16-slot frame with the deferred list behind it ---------------------------------
_QUAD_ORDINARY = [n for n in nc.QUAD_W + nc.QUAD_H if nc.SPECS[n]["nprob"] < 1000]


@pytest.mark.parametrize("name", _QUAD_ORDINARY)
def test_quad_frame32(name):
    _run(name, {"nnqp_quad": 2, "nnqp_frame16": 0}, tag="|quad32")


@pytest.mark.parametrize("name", _QUAD_ORDINARY)
def test_quad_frame16_then_list(name):
    _run(name, {"nnqp_quad": 2, "nnqp_frame16": 1}, prime=True, tag="|quad16+list")


def test_quad_grid_stride_frame32():
    """8 192 + 16 + 3 problems: the 512 workgroups x 16 problems of the 32-slot launch and one partial sweep."""
    _run("w_k48_grid32", {"nnqp_quad": 2, "nnqp_frame16": 0}, tag="|quad32")


@pytest.mark.parametrize("count", [0, 1])
def test_quad_grid_stride_frame16(count):
    """12 288 + 48 + 3 problems from the exact support: the 256 workgroups x 48 problems of the 16-slot launch and one partial
    sweep.  The 16-slot frame solves the 7 594 problems with s <= 16 (31 of the 51 in the partial sweep) and lists the 4 745
    with s > 16 (20 of the 51), which the 32-slot launch behind solves.  count = 0: the production instantiations; count = 1:
    the counting ones, whose counters must show exactly that split."""
    cnt = _run("w_k48_grid16", {"nnqp_quad": 2, "nnqp_frame16": 1, "nnqp_count": count}, prime=True,
               tag="|quad16+list" + ("|counted" if count else ""))
    if count:
        _assert_split(nc.case("w_k48_grid16"), cnt, "w_k48_grid16|quad16+list|counted")


@pytest.mark.parametrize("k", nc.QUAD_K)
def test_quad_frame16_ran_behind_the_priming_step(k):
    """The "|quad16+list" items rest on the zero-data priming step leaving a history that sends the next half step to the
    16-slot frame; both frames return the same bits, so the results cannot show it.  One counted item per k does."""
    name = "w_k%d_support" % k
    cnt = _run(name, {"nnqp_quad": 2, "nnqp_frame16": 1, "nnqp_count": 1}, prime=True, tag="|quad16+list|counted")
    _assert_split(nc.case(name), cnt, name + "|quad16+list|counted")


def test_quad_default_switch():
    """16 384 + 5 problems with the options left alone: the half step goes to k_nnqp_quad by the default rule."""
    c = nc.case("w_k64_default")
    ctx = _context(c, {"nnqp_count": 1})
    try:
        x = _half_step(ctx, c)
        cnt = ctx.nnqp_counters(reset=True)
    finally:
        ctx.close()
    assert cnt["frame16"]["problems"] + cnt["frame32"]["problems"] == c.nprob, cnt
    _check(c, x, c.name + "|default")


# ---- k_nnqp (one lane per variable): the same cases with the quad kernel off ------------------------------------------------------
@pytest.mark.parametrize("name", _QUAD_ORDINARY)
def test_lane_per_variable(name):
    _run(name, {"nnqp_quad": 0}, tag="|lane")


# ---- k_nnqp_wave (65 .. 128 bases) and k_nnqp_big -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.WAVE)
def test_wave(name):
    _run(name, {}, tag="|wave")


@pytest.mark.parametrize("name", nc.BIG)
def test_big(name):
    _run(name, {"nnqp_wave": 0}, tag="|big")


# ---- the conditioning ladder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.LADDERS)
def test_ladder_quad(name):
    """Pivot ratios 1e-3, 1e-5, 1e-7: inside the flag's 1e-8, so k_nnqp_quad solves them (its counters say so) -- a problem
    that ran into the pass limit would come back with a wrong support or outside bound_x."""
    c = nc.case(name)
    ctx = _context(c, {"nnqp_quad": 2, "nnqp_count": 1})
    try:
        x = _half_step(ctx, c)
        cnt = ctx.nnqp_counters(reset=True)
    finally:
        ctx.close()
    assert cnt["frame16"]["problems"] + cnt["frame32"]["problems"] == c.nprob, cnt
    print("%s: passes per wave task %.2f" % (name, cnt["frame32"]["passes"] / max(cnt["frame32"]["wave_tasks"], 1)))
    _check(c, x, name + "|quad32")


@pytest.mark.parametrize("name", nc.LADDERS)
def test_ladder_quad_frame16(name):
    _run(name, {"nnqp_quad": 2}, prime=True, tag="|quad16+list")


@pytest.mark.parametrize("name", nc.LADDERS)
def test_ladder_lane_per_variable(name):
    _run(name, {"nnqp_quad": 0}, tag="|lane")


# ---- the frame hand-over --------------------------------------------------------------------------------------------------------
def test_frame_sequence_counts_every_problem_once():
    """Four W half steps of one context on four planted data sets, exact-support start: the first solve of a problem is its
    last (k_nnqp_quad: a problem is deferred in the pass that finds its system beyond the frame, before any exchange, and
    with P planted nothing is infeasible after the first solve), so the 32-slot frame solves exactly the planted number of
    problems with s > 16 whenever the 16-slot frame ran, and everything when it did not."""
    seq = nc.sequence()
    c0 = seq[0]
    ctx = _context(c0, {"nnqp_quad": 2, "nnqp_frame16": 1, "nnqp_count": 1})
    try:
        ctx.set_h(c0.factor)
        ctx.nnqp_counters(reset=True)
        for step, c in enumerate(seq):
            ctx.set_v_dense(c.V)
            ctx.set_w(c.X0)
            ctx.update_w()
            x = ctx.get_w()
            cnt = ctx.nnqp_counters(reset=True)
            s16, s32 = cnt["frame16"]["problems"], cnt["frame32"]["problems"]
            nbig = int((c.sys_size() > 16).sum())
            print("step %d: solved16 = %d, solved32 = %d, planted s > 16: %d of %d" % (step + 1, s16, s32, nbig, c.nprob))
            assert s16 + s32 == c.nprob, (step, cnt)
            if step in (1, 2):         # the decision read a share <= 10 %: the 16-slot frame ran and listed the big ones
                assert s32 == nbig, (step, cnt)
            else:                      # no history / 50 % beyond the frame: everything on the 32-slot frame
                assert s16 == 0 and s32 == c.nprob, (step, cnt)
            _check(c, x, c.name)
    finally:
        ctx.close()


# ---- the device-side fallback: HA singular ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, opts", [(24, {"nnqp_quad": 2, "nnqp_count": 1}), (100, {})])
def test_fallback_on_singular_hessian(k, opts):
    """H row 7 = row 3: the flag is 0, k_nnqp_quad / k_nnqp_wave return at once and k_nnqp / k_nnqp_big take the half step
    from a cold start.  The minimiser is not unique: KKT and the objective, with bounds from the float64 problem -- the device
    minimises with f_dev, |f_dev - f| <= eps_f, and stores fl32(x): w = f - HA x <= eps_f + 2^-24 |HA| x, and
    0 <= q(x_dev) - q(x*) <= eps_f' (x_dev + x*) + 2^-24 x_dev' (|HA| x_dev + |f|).  At k = 24 the counting instantiations
    of k_nnqp_quad run: they must have started no wave task and solved nothing (test_ladder_quad and test_quad_default_switch
    show the same counters at nprob when the flag is 1), so the result is k_nnqp's."""
    fb = nc.fallback(k)
    ctx = _lib.Context(_lib.ALGO_NMFALS, fb["nprob"], fb["ln"], k)
    try:
        for name, value in opts.items():
            ctx.set_option(name, value)
        ctx.set_v_dense(fb["V"])
        ctx.set_w(np.ones((fb["nprob"], k), dtype=np.float32))
        ctx.set_h(fb["H"])
        ctx.update_w()
        x = ctx.get_w().astype(np.float64)
        cnt = ctx.nnqp_counters(reset=True)
    finally:
        ctx.close()
    assert not any(cnt[fr][key] for fr in cnt for key in cnt[fr]), cnt
    HA, f, ef = fb["HA"], fb["f64"], fb["eps_f"]
    assert np.isfinite(x).all() and (x >= 0).all()
    w = f - x.dot(HA)
    tol_w = ef + 2.0 ** -24 * x.dot(np.abs(HA)) + 1e-12 * np.abs(f).max()
    assert (w <= tol_w).all(), float((w - tol_w).max())
    assert (np.abs(x * w) <= x * tol_w).all()
    worst = 0.0
    for i in range(fb["nprob"]):
        xs = nnqp_solve(HA, -f[i])
        q = lambda v: 0.5 * v.dot(HA).dot(v) - f[i].dot(v)
        gap = q(x[i]) - q(xs)
        tol_q = ef[i].dot(x[i] + xs) + 2.0 ** -24 * x[i].dot(np.abs(HA).dot(x[i]) + np.abs(f[i]))
        worst = max(worst, abs(gap) / tol_q)
        assert -1e-9 * abs(q(xs)) - 1e-9 <= gap <= tol_q, (i, gap, tol_q)
    print("fallback k = %d: worst objective gap / bound = %.3e" % (k, worst))
    _fallback["fallback_k%d" % k] = worst
