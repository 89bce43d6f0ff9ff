#!/usr/bin/env python3
"""Generate the SIVM_GSAT golden vectors (tests/golden/gsat_*.npz) by running the REAL reference pymf/sivm_gsat.py (with
sivm.py, aa.py, vol.py and dist.py behind it), unmodified, through the shims of gen_golden.py, gen_golden_sivm.py (the cvxopt
stand-in: H and ferr pin aa.py's data flow, not cvxopt's digits) and gen_golden_sgreedy.py (scipy.misc.factorial, scipy.inf).

The module is Python 2 code; three more stand-ins are installed before it is imported or used, none of which touches its text:
  np.int   -> int                      (sivm_gsat.py:120; removed from NumPy)
  xrange   -> range                    (builtins; sivm_gsat.py:168, dist.py:112)
  range    -> a list-returning range   as a global of the imported module alone: init_w keeps `range(num_bases)` as `select`
                                       and update_w assigns select[s] = n (sivm_gsat.py:79,124), which needs Python 2's list
Only inputs and results are stored: the drawn indices, the verdict per probe (the slot replaced, -1 rejected, -2 skipped by
`n not in select`), the final select, W, _v, V (as vol), the decision margin min over probes of |max_i v[i] - V| / V, and H and ferr
where computed.  The verdicts and margins are observed by wrapping online_update_w and cmdet from outside.
The reference is fed float64 arrays holding float32-representable values."""
import builtins
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden_sgreedy import load_sgreedy  # noqa: E402
import gsat_cases as gc  # noqa: E402


def load_gsat():
    if not hasattr(np, "int"):
        np.int = int
    builtins.xrange = range
    load_sgreedy()
    mod = importlib.import_module("pymf.sivm_gsat")
    mod.range = lambda *a: list(builtins.range(*a))
    return mod


def run(mod, V, k, measure, seed, niter, compute_h, W=None, compute_w=True):
    """One seeded factorize(niter) of the reference; the probes' indices, verdicts and the decision margin observed from outside"""
    mdl = mod.SIVM_GSAT(V.astype(np.float64), num_bases=k, dist_measure=measure)
    if W is not None:
        mdl.W = W.copy()
    n = V.shape[1]
    idx = np.floor(np.random.RandomState(seed).random_sample(niter) * n).astype(np.int64)
    slots, state = [], {"margin": np.inf, "vols": None}
    inner, cmdet = mdl.online_update_w, mod.cmdet

    def online(vec):
        state["vols"] = []
        updated, s = inner(vec)
        vols = state["vols"][-k:]                              # (the first probe also computes V: the k leave-one-out volumes are the last)
        state["vols"] = None
        Vb = mdl._v[-2] if updated else mdl.V                  # the volume the probe was compared with
        state["margin"] = min(state["margin"], abs(max(vols) - Vb) / Vb if Vb > 0 else 0.0)
        slots.append(int(s))
        return updated, s

    def counted(d):
        v = cmdet(d)
        if state["vols"] is not None:
            state["vols"].append(float(v))
        return v

    mdl.online_update_w = online
    mod.cmdet = counted
    try:
        np.random.seed(seed)

        def update_w():                                        # a probe that `n not in select` turns away reaches no online_update_w
            n_before = len(slots)
            type(mdl).update_w(mdl)
            if len(slots) == n_before:
                slots.append(-2)
        mdl.update_w = update_w
        mdl.factorize(niter=niter, compute_w=compute_w, compute_h=compute_h, compute_err=compute_h)
    finally:
        mod.cmdet = cmdet
    d = dict(k=np.int64(k), measure=np.str_(measure), seed=np.int64(seed), niter=np.int64(niter), W=np.asarray(mdl.W, dtype=np.float64))
    if compute_w:
        assert len(slots) == niter
        d.update(idx=idx, slots=np.asarray(slots, dtype=np.int64), select=np.asarray(mdl.select, dtype=np.int64),
                 v=np.asarray(getattr(mdl, "_v", []), dtype=np.float64), vol=np.float64(getattr(mdl, "V", np.nan)), margin=np.float64(state["margin"]))
        assert [int(s) for s in d["select"]] == replay(d["idx"], d["slots"], k), "the drawn indices are not the stored ones"
    if compute_h:
        d.update(H=np.asarray(mdl.H, dtype=np.float64), ferr=np.asarray(mdl.ferr, dtype=np.float64), H_is_data_flow_pin=np.bool_(True))
    return d


def replay(idx, slots, k):
    sel = list(range(k))
    for n, s in zip(idx, slots):
        if s >= 0:
            sel[int(s)] = int(n)
    return sel


def main():
    mod = load_gsat()
    cases = {}
    Vd = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]], dtype=np.float32)                      # sivm_gsat.py:60-63
    cases["gsat_doc_2x3_k2"] = dict(run(mod, Vd, 2, "l2", 4, 1, True), V=Vd)
    Vu = np.array([[1.5, 1.3], [1.2, 0.3]], dtype=np.float32)                                # sivm_gsat.py:69-73
    cases["gsat_doc_userw"] = dict(run(mod, Vu, 2, "l2", 3, 1, True, W=np.array([[1.0, 0.0], [0.0, 1.0]]), compute_w=False), V=Vu)
    for name in gc.GOLDEN_CASES:                               # (beyond 35 bases the reference's f1 is 0: gsat_cases.py)
        s = gc.spec(name)
        cases[name] = dict(run(mod, gc.data(name), s["k"], s["measure"], s["seed"], s["niter"], False), case=np.str_(name))
    s = gc.spec(gc.H_CASE)
    cases[gc.H_CASE + "_h"] = dict(run(mod, gc.data(gc.H_CASE), s["k"], s["measure"], s["seed"], 3, True), case=np.str_(gc.H_CASE))

    for name, d in cases.items():
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
        if "slots" in d:
            print("%-24s swaps %3d skipped %3d per batch %s margin %.3e vol %.6g select %s" % (
                name, int((d["slots"] >= 0).sum()), int((d["slots"] == -2).sum()), gc.swaps_per_batch(d["slots"]), float(d["margin"]),
                float(d["vol"]), d["select"][:8]))


if __name__ == "__main__":
    main()
