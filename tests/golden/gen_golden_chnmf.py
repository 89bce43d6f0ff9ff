#!/usr/bin/env python3
"""Generate the CHNMF golden vectors (tests/golden/chnmf_*.npz) by running the REAL reference pymf/chnmf.py, imported unmodified
through the shims of gen_golden.py (xrange) and gen_golden_aa.py (the exact-minimiser stand-in for cvxopt, see there: the
goldens pin the data flow of chnmf.py and aa.py, not an interior-point solver's digits).

Every case runs under a fixed np.random.seed: the first draw of CHNMF.factorize is R = np.random.randn(base_sel, rows)
(chnmf.py:180; init_w and init_h of CHNMF draw nothing), the nested AA draws its start afterwards.  R is recorded by drawing it
again from the same seed.  A case is written only if it is determinate in the sense of tests/chnmf_cases.py (every hull vertex,
every interior point and every pair of distinct points clear of rounding by 1e4 gamma) and if the monotone chain restated there
gives the reference's _hull_idx.  The reference is fed float64 arrays holding float32-representable values.

One more shim, on the module's own `np` name: quickhull's `dists` (chnmf.py:44) is np.dot of 2-vectors.  Where NumPy's BLAS
fuses multiply and add, the pivot's own distance to the edge it ends -- (a, b) . (-b, a) -- comes out as the rounding error of
a b instead of 0; when that is positive the pivot is "outside" its own edge, is chosen again, and dome() never returns
(RecursionError on most inputs, the three points of the docstring among them).  The stand-in evaluates np.dot with a vector
operand as separately rounded products added up, which makes that distance exactly 0 as the reference assumes.  The product
of two matrices (proj = R data, chnmf.py:181) is evaluated entry by entry in ONE summation order (np.einsum): a blocked BLAS
sums a column by its position, so that identical data columns project to points a rounding error apart and the reference's
"first index among duplicates" (vq, chnmf.py:167) becomes a coin toss; in one order they project to one point."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden_aa import load_aa  # noqa: E402
import chnmf_cases as cc  # noqa: E402


class _UnfusedDot(object):
    """numpy, except for dot: a 1-D operand: every product rounded before it is added; two matrices: one summation order."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def dot(a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.ndim == 2 and b.ndim == 2:
            return np.einsum("sr,rc->sc", a, b)
        return (a * b).sum(axis=-1)


def ring_data(seed, rows, n, on_hull):
    """rows x n data whose projection by the R of `seed` (2 x rows) is: on_hull points on the unit circle -- all of them hull
    vertices --, the others inside it on distinct radii in [0.3, 0.999], in shuffled order."""
    np.random.seed(seed)
    R = np.random.randn(2, rows)
    rs = np.random.RandomState(seed + 1)
    ang = 2.0 * np.pi * (np.arange(n) + rs.random_sample(n) * 0.5) / n
    rad = np.linspace(0.3, 0.999, n)
    rs.shuffle(rad)
    rad[rs.choice(n, on_hull, replace=False)] = 1.0
    P = np.stack([rad * np.cos(ang), rad * np.sin(ang)])
    Rpinv = np.linalg.pinv(R)
    null = np.eye(rows) - Rpinv.dot(R)                          # what R does not see
    V = Rpinv.dot(P) + null.dot(rs.random_sample((rows, n)))
    return V.astype(np.float32)


def main():
    load_aa()
    chnmf = importlib.import_module("pymf.chnmf")
    chnmf.np = _UnfusedDot()
    cases = {}

    def add(name, V, k, base_sel, seed):
        V = np.ascontiguousarray(V, dtype=np.float32)
        np.random.seed(seed)
        mdl = chnmf.CHNMF(V.astype(np.float64), num_bases=k, base_sel=base_sel)
        mdl.factorize()
        np.random.seed(seed)
        R = np.random.randn(mdl._base_sel, V.shape[0])
        hull = np.asarray(mdl._hull_idx, dtype=np.int32)
        outer, inner, sep, tau = cc.margins(V, R)
        print("%-28s hull %4d  vertex margin %.3e  interior margin %.3e  separation %.3e  tau %.3e  ferr %s" % (
            name, hull.shape[0], outer, inner, sep, tau, mdl.ferr))
        assert outer > tau and inner > tau and sep > tau, "not determinate"
        assert np.array_equal(cc.hull_union(V, R), hull), "the monotone chain disagrees with the reference's quickhull"
        cases[name] = dict(V=V, seed=np.int64(seed), k=np.int64(k), base_sel=np.int64(mdl._base_sel), R=R, _hull_idx=hull,
                           W=np.asarray(mdl.W, dtype=np.float64), H=np.asarray(mdl.H, dtype=np.float64),
                           ferr=np.asarray(mdl.ferr, dtype=np.float64), Wmapped_index=np.asarray(mdl._Wmapped_index, dtype=np.int64))
        return mdl

    add("chnmf_doc_2x3_k2", np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]]), 2, 3, 7)          # chnmf.py:98-106
    V29 = np.random.RandomState(29300).random_sample((29, 300))
    base = add("chnmf_29x300_k6_sel3", V29, 6, 3, 11)
    add("chnmf_37x1061_k5_sel5", np.random.RandomState(371061).random_sample((37, 1061)), 5, 5, 12)
    add("chnmf_8x5000_k4_sel2_ring", ring_data(13, 8, 5000, 400), 4, 2, 13)
    # ten columns duplicated, two of them hull vertices of the case above (same seed, same R): one copy below its original,
    # one above; the other eight copies are interior columns
    Vd = V29.astype(np.float32).copy()
    hull = [int(h) for h in base._hull_idx]
    inner = [c for c in range(300) if c not in hull]
    v_hi, v_lo = max(hull), min(h for h in hull if h > 0)
    lo_slot = max(c for c in inner if c < v_hi and c != v_lo)
    Vd[:, inner[-1]] = Vd[:, v_lo]                              # copy ABOVE its original: the original's index stays
    Vd[:, inner[0] if inner[0] < v_hi else lo_slot] = Vd[:, v_hi]   # copy BELOW its original: the copy's index enters
    for q in range(8):
        Vd[:, inner[-2 - q]] = Vd[:, inner[10 + q]]
    mdl = add("chnmf_29x300_dups", Vd, 6, 3, 11)
    groups = {}
    for c in range(300):
        groups.setdefault(Vd[:, c].tobytes(), []).append(c)
    dup_groups = [g for g in groups.values() if len(g) > 1]
    on_hull = [g for g in dup_groups if set(g) & set(int(h) for h in mdl._hull_idx)]
    assert len(dup_groups) == 10 and len(on_hull) >= 2, (len(dup_groups), len(on_hull))
    for g in on_hull:
        assert [c for c in g if c in set(int(h) for h in mdl._hull_idx)] == [min(g)], g
    cases["chnmf_29x300_dups"]["dup_vertices"] = np.array([min(g) for g in on_hull], dtype=np.int64)

    for name, d in cases.items():
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)


if __name__ == "__main__":
    main()
