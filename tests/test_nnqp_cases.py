"""The planted problems of tests/nnqp_cases.py are well-posed -- checked here in float64, without a device: the planted support
survives a float32 right-hand side with a factor 2 to spare, the recomputed reference satisfies KKT, the float64 oracle finds
the same minimiser, and every named edge (passive-set size, frame share, conditioning rung) occurs."""
import numpy as np
import pytest

import nnqp_cases as nc
from oracle.nmfals_oracle import nnqp_solve


def _check_case(c):
    P, live = c.P, c.live
    N = ~P & live[None, :]
    # the planted support survives float32: margins of 2 bounds on both sides
    xm = np.where(P, c.x_ref, np.inf).min(axis=1)
    wm = np.where(N, -c.w_ref, np.inf).min(axis=1)
    assert (xm > 2.0 * c.bound_x).all(), (c.name, float(np.min(xm / np.maximum(c.bound_x, 1e-300))))
    assert (wm > 2.0 * c.bound_w).all(), (c.name, float(np.min(wm / np.maximum(c.bound_w, 1e-300))))
    # KKT in float64: x >= 0, w = f - HA x zero on P and negative on N, complementary
    w = c.f64 - c.x_ref.dot(c.HA)
    scale = np.abs(c.f64).max() + 1.0
    assert (c.x_ref >= 0).all() and (c.x_ref[~P] == 0).all()
    assert np.abs(np.where(P, w, 0.0)).max() <= 1e-10 * scale
    assert np.abs(np.where(N, w - c.w_ref, 0.0)).max() <= 1e-10 * scale
    assert (np.where(N, w, -1.0) < 0).all()


def _check_oracle(c, nsample):
    # the float64 active-set oracle ends at the same support and point (a sample that covers every size first)
    sizes = c.P.sum(axis=1)
    first = [int(np.flatnonzero(sizes == s)[0]) for s in np.unique(sizes)]
    rest = [i for i in range(0, c.nprob, max(1, c.nprob // nsample)) if i not in first]
    for i in (first + rest)[:nsample]:
        x = nnqp_solve(c.HA, -c.f64[i])
        assert ((x > 0) == c.P[i]).all(), (c.name, i)
        assert np.abs(x - c.x_ref[i]).max() <= 1e-10 * max(np.abs(c.x_ref[i]).max(), 1.0), (c.name, i)


def _nsample(k):
    return 64 if k <= 64 else 8 if k <= 128 else 2       # (the oracle borders one variable at a time: O(k^4) per problem)


@pytest.mark.parametrize("name", sorted(nc.SPECS))
def test_case_is_well_posed(name):
    c = nc.case(name)
    spec = nc.SPECS[name]
    assert c.nprob % 4 != 0 and c.nprob % 48 != 0
    assert nc.min_pivot_ratio(c.HA) > nc.FLAG_MIN_PIVOT          # the fast kernels take it (flag = 1)
    _check_case(c)
    _check_oracle(c, _nsample(c.k) if c.nprob < 1000 else 16)
    if spec["kind"] != "ladder":
        have = set(int(s) for s in c.P.sum(axis=1))
        assert have == set(nc.sizes_of(spec)), (name, sorted(have))
        # every size meets every position rule
        seen = set((int(c.P[i].sum()), nc.POSITIONS[i % 5]) for i in range(c.nprob))
        assert len(seen) == len(have) * 4


def test_size_lists_hold_the_edges():
    assert nc.quad_sizes(64) == [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
    assert nc.quad_sizes(48) == [0, 1, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48]
    assert nc.SPECS["w_k48_grid16"]["start"] == "support"
    g = nc.case("w_k48_grid16")
    big = g.sys_size() > 16
    # both sweeps of the 16-slot launch (256 workgroups x 48 problems, then the partial one) hold work for both frames
    assert big.sum() == 4745 and 0 < big[12288:].sum() < big[12288:].size and ((g.X0 > 0) == g.P).all()
    assert nc.quad_sizes(1) == [0, 1] and nc.quad_sizes(17) == [0, 1, 2, 7, 8, 9, 15, 16, 17]
    assert nc.wave_sizes(128) == [0, 1, 63, 64, 65, 127, 128] and nc.wave_sizes(65) == [0, 1, 63, 64, 65]
    for k in nc.QUAD_K + nc.WAVE_K:
        for sizes in (nc.quad_sizes(k), nc.wave_sizes(k), nc.lane_sizes(k)):
            n = len(nc.size_cycle(sizes))
            assert n % 2 and n % 3 and n % 5 and set(nc.size_cycle(sizes)) == set(sizes)
    # the frame boundary from both sides at every k that has it
    for k in (33, 47, 48, 49, 63, 64):
        s = set(min(p, k - p) for p in nc.quad_sizes(k))
        assert {16, 17} <= s or k < 34, (k, sorted(s))


def test_wave_cases_hold_supports_inside_one_half():
    """A lane of k_nnqp_wave owns variables t and t + 64: supports wholly below 64 and wholly from 64 on."""
    for name in nc.WAVE:
        c = nc.case(name)
        lo = [i for i in range(c.nprob) if c.P[i].any() and not c.P[i, 64:].any() and c.P[i].sum() >= 63]
        hi = [i for i in range(c.nprob) if c.P[i].any() and not c.P[i, :64].any()]
        assert lo and hi, name
        if c.k > 65:
            assert max(int(c.P[i].sum()) for i in hi) == c.k - 64, name


def test_dead_basis_case():
    c = nc.case("w_k48_dead")
    assert not c.live[5] and c.live.sum() == 47 and (c.factor[5] == 0).all()
    assert (c.X0[:, 5] == 1).all() and not c.P[:, 5].any()


def test_h_step_hessian_is_exact_in_float32():
    for name in nc.QUAD_H + [n for n in nc.WAVE if nc.SPECS[n]["step"] == "h"]:
        c = nc.case(name)
        assert (c.HA.astype(np.float32).astype(np.float64) == c.HA).all() and np.abs(c.HA).max() < 2 ** 24
        assert (c.HA == np.round(c.HA)).all()


@pytest.mark.parametrize("name", nc.LADDERS)
def test_ladder_rung_is_where_it_says(name):
    c = nc.case(name)
    target = float(nc.SPECS[name]["rung"])
    ratio = nc.min_pivot_ratio(c.HA)
    assert 0.5 * target <= ratio <= 2.0 * target, ratio
    assert ratio > nc.FLAG_MIN_PIVOT
    # HA is exact in float64: the factor's entries are multiples of 2^-18 below 8, so HA 2^36 is an integer below 2^53
    F = c.factor.astype(np.float64)
    assert (F * 2.0 ** 18 == np.round(F * 2.0 ** 18)).all() and np.abs(F).max() < 8
    assert (c.HA * 2.0 ** 36 == np.round(c.HA * 2.0 ** 36)).all() and np.abs(c.HA).max() * 2.0 ** 36 < 2.0 ** 53
    # the rung's reach: problems that cross an ill-conditioned HA[P,P] (the pair passive together) on the way
    assert (c.X0 == 0).all()
    nenter = nc.pair_enters_first(c).size
    assert nenter >= (10 if c.k == 32 else 40), nenter
    i, j = nc.LADDER_PAIR
    assert not c.P[:, i].any() and not c.P[:, j].any()
    sizes = c.P.sum(axis=1)
    assert sizes.min() <= 2 and sizes.max() >= c.k - 2           # random supports of every size


def test_frame_sequence_shares():
    seq = nc.sequence()
    assert len(seq) == 4
    for c, share in zip(seq, nc.SEQ_SHARES):
        _check_case(c)
        _check_oracle(c, 16)
        s = c.sys_size()
        nbig = int((s > 16).sum())
        assert abs(nbig - share * c.nprob) < 1.0, (c.name, nbig)
        assert s.max() <= 24 and (c.X0 > 0).tolist() == c.P.tolist()
        assert (seq[0].factor == c.factor).all()
    # what the device decides from: more than a tenth of the previous step's problems beyond 16 unknowns
    n = nc.SEQ_NPROB
    assert 10 * int((seq[1].sys_size() > 16).sum()) <= n < 10 * int((seq[2].sys_size() > 16).sum())


@pytest.mark.parametrize("k", [24, 100])
def test_fallback_hessian_is_singular(k):
    fb = nc.fallback(k)
    assert (fb["H"][7] == fb["H"][3]).all()
    assert nc.min_pivot_ratio(fb["HA"]) <= 0.0                    # exactly: row 7's pivot is 0 in exact arithmetic, HA is exact
    x = nnqp_solve(fb["HA"], -fb["f64"][0])
    assert (x >= 0).all() and np.isfinite(x).all()
