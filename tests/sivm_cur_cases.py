"""The device cases of SIVM_CUR (tests/test_gpu_sivm_cur.py) and what makes the comparison with the float64 oracle meaningful
(tests/test_sivm_cur_cases.py, no GPU): the smallest shapes at which the long-sample pass (k_sivm_rowdist, k_sivm_rowstep), the
column-panel pass behind pmf_sivm_select and the paths between them can go wrong.

The oracle is sivm_oracle.update_w on d.T (the rows) and on d (the columns), then cur_oracle.compute_ucr and gram_form.

Data are (randn(m, r) linspace(3, 0.3, r)) randn(r, n) / sqrt(r) with r = min(m, n), float32 (greedy_cases.spectrum_data): a
decaying spectrum in both directions, so that rows and columns alike have clear extremes; `scale` and `offset` rescale and
shift them (all values stay float32-representable).  Planted-vertex data (sivm_cases.planted) give an argmax gap among the
columns only.  The seed of every case is the first one, counting up from the seed named in SEARCH_FROM, at which EVERY argmax of
both selections -- the two intermediate ones of the 'fastmap' start included -- keeps a gap (best - second) / (best - median) of
at least sivm_cases.MIN_GAP in float64 and with every distance rounded to float32, both runs select the same indices, and the
kept eigenvalues of C^T C and R R^T satisfy the condition tests/test_cur_cases.py holds CUR to (tools: `python
tests/sivm_cur_cases.py` repeats the search and prints the seeds and the figures below).

Two argmaxes cannot have a gap and are held to what they are instead (tests/test_sivm_cur_cases.py):
  * 'cosine' under 'origin': every candidate is at distance 1 - 0 / (0 + 1e-9) = 1 from the origin, so the first recurrence
    round scores all candidates alike, bit for bit, and the lowest index, 0, is taken (by np.argmax and by the device);
  * the tie case: row TIE_SRC, the winner of round TIE_ROUND of the row selection, is copied to the higher index TIE_DUP.
    That round is an exact tie of the two (the gap is taken to the third); the lower index wins and the copy, at distance 0
    from a chosen row ever after, is never chosen.
"""
import numpy as np

import cur_oracle as co
import sivm_cases as sc
import sivm_oracle as so

SLAB = 2048              # PMF_SIVM_SLAB (pymf_amd/csrc/pmf_sivm.h): columns per slab of the long-sample pass
ROWS_WG = 32             # PMF_SIVM_ROWS_WG: rows per workgroup
MAX_BASES = 64
FACTOR = 4.0             # device tolerance = FACTOR x the oracle-vs-twin deviation (cur_cases.py, greedy_cases.py)

# name: (rows, cols, rrank, seed, offset, scale, metric, init)
CASES = {
    "doc_2x3": (2, 3, 1, None, 0.0, 1.0, "l2", "origin"),                  # sivm_cur.py:55-57: both lists are [-1]
    "5x37": (5, 37, 3, 1, 0.0, 1.0, "l2", "origin"),                       # one partial slab, rows no multiple of 4, fewer rows than a wave
    "29x300_l2": (29, 300, 6, 2, 0.0, 1.0, "l2", "origin"),
    "29x300_l1": (29, 300, 6, 6, 0.0, 1.0, "l1", "origin"),
    "29x300_cosine": (29, 300, 6, 52, 0.0, 1.0, "cosine", "origin"),
    "29x300_fastmap": (29, 300, 6, 6, 0.0, 1.0, "l2", "fastmap"),
    "29x300_offset1000": (29, 300, 6, 8, 1000.0, 100.0, "l2", "origin"),   # distances from differences
    "40x4133": (40, 4133, 8, 7, 0.0, 1.0, "l2", "origin"),                 # slabs of 2048: 2048 + 2048 + 37 columns, the last quad ragged
    "300x29": (300, 29, 6, 9, 0.0, 1.0, "l2", "origin"),                   # tall: 10 row blocks (the last: 12 rows), rows shorter than one 64-lane read
    "130x2100": (130, 2100, 20, 9, 0.0, 1.0, "l2", "origin"),              # 5 row blocks (the last: 2 rows) x 2 slabs
    "64x2048_r64": (64, 2048, 64, 220, 0.0, 1.0, "l2", "origin"),           # the limit
    "40x300_tie": (40, 300, 5, 11, 0.0, 1.0, "l2", "origin"),              # row TIE_SRC copied to TIE_DUP
}
SEARCH_FROM = {"5x37": 1, "29x300_l2": 2, "29x300_l1": 3, "29x300_cosine": 4, "29x300_fastmap": 5, "29x300_offset1000": 6,
               "40x4133": 7, "300x29": 8, "130x2100": 9, "64x2048_r64": 10, "40x300_tie": 11}
TIE_CASE = "40x300_tie"
TIE_ROUND = 2            # select[2] of the row selection
GOLDEN = ("doc_2x3", "29x300_l2", "300x29", "29x300_cosine_fastmap")
GOLDEN_ONLY = {"29x300_cosine_fastmap": (29, 300, 6, 12, 0.0, 1.0, "cosine", "fastmap")}
SEARCH_FROM["29x300_cosine_fastmap"] = 12

# The oracle-vs-twin deviations measured on the cases above (tests/test_sivm_cur_cases.py re-measures them per case and holds
# them to these figures): max |U_twin - U| / max |U| (the twin's middle factor is the Gram form of cur_oracle.gram_form on the
# float32 data) and |ferr_twin - ferr| / ||data|| (the larger of cur_oracle.twin's and of twin_ferr's below, which also rounds the
# squares of the residual as the device's residual pass does), each with the case that produced it.
TWIN_U_DEV = 1.24e-10    # 64x2048_r64 (1.237e-10; 3.5e-13 at 29x300_offset1000, below 5e-14 everywhere else)
TWIN_FERR_DEV = 9.8e-9    # doc_2x3 (9.77e-09, all of it the float32 squares of the residual pass: twin_ferr; 4.6e-09 at 5x37, below 2.5e-09 everywhere else)

_DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])
_cache = {}


def _spec(name):
    return CASES.get(name) or GOLDEN_ONLY[name]


def spectrum_data(rows, cols, seed, offset=0.0, scale=1.0):
    rng = np.random.RandomState(seed)
    r = min(rows, cols)
    d = np.dot(rng.randn(rows, r) * np.linspace(3.0, 0.3, r), rng.randn(r, cols)) / np.sqrt(r)
    return (offset + scale * d).astype(np.float32)


def tie_rows(d, rrank, metric, init):
    """(source, duplicate): the winner of round TIE_ROUND of the row selection and a higher row index, not selected, that
    receives its copy."""
    sel, _ = so.update_w(d.astype(np.float64).T, rrank, metric, init)
    src = sel[TIE_ROUND]
    dup = max(r for r in range(d.shape[0]) if r > src and r not in sel and r != d.shape[0] - 1)
    return src, dup


def data(name, seed=None):
    """float32 data of a case."""
    rows, cols, rrank, s, offset, scale, metric, init = _spec(name)
    if name == "doc_2x3":
        return _DOC.astype(np.float32)
    d = spectrum_data(rows, cols, s if seed is None else seed, offset, scale)
    if name == TIE_CASE:
        src, dup = tie_rows(d, rrank, metric, init)
        d[dup, :] = d[src, :]
    return d


def REPLACED_DATA():
    """29 x 300 data that replace those of 29x300_l2 in place (tests/test_gpu_sivm_cur.py): those of another case."""
    return data("29x300_fastmap")


def all_scores(V, k, metric, init, f32_dist=False):
    """(select, scores): sivm_oracle.update_w with the score vector of EVERY argmax -- under 'fastmap' the two intermediate
    distance passes, which update_w does not hand back, come first."""
    V = np.asarray(V, dtype=np.float64)
    scores = []
    if init == "fastmap":
        cur = 0
        for _ in range(2):
            d = so.distance(V, cur, metric)
            d = so.f32(d) if f32_dist else d
            scores.append(d.copy())
            cur = int(np.argmax(d))
    tail = []
    select, _ = so.update_w(V, k, metric, init, f32_dist=f32_dist, scores=tail)
    return select, scores + tail


def chosen_before(select, init, j):
    """The candidates already selected when argmax number j of all_scores is taken."""
    first = 2 if init == "fastmap" else -1       # 'fastmap': argmax 2 finds select[0]; 'origin': argmax 0 finds select[1]
    return [s for s in select[:max(j - first, 0)] if s >= 0]


def gaps(scores, select, init):
    """Per argmax (best - second) / (best - median) and (best - third) / (best - median), sivm_cases' measure.  Once half of
    the candidates are chosen (64 rows of 64) the median is itself a chosen candidate, whose score lies a multiple of
    log(1e-8) below every other, and the measure says nothing any more: the median is then taken over the candidates not yet
    chosen.  An all-equal vector gives (0, 0)."""
    out = []
    for j, s in enumerate(scores):
        o = np.sort(s)[::-1]
        done = chosen_before(select, init, j)
        med = np.median(s) if 2 * len(done) < len(s) else np.median(np.delete(s, done))
        spread = o[0] - med
        if len(o) < 2 or spread == 0.0:
            out.append((0.0 if len(o) > 1 else 1.0, 0.0 if len(o) > 2 else 1.0))
        else:
            out.append((float((o[0] - o[1]) / spread), float((o[0] - o[2]) / spread) if len(o) > 2 else 1.0))
    return out


def expected_ties(name):
    """{(side, argmax number): kind}: the argmaxes of a case that are ties by construction (module docstring)."""
    rows, cols, rrank, _, _, _, metric, init = _spec(name)
    t = {}
    if metric == "cosine" and init == "origin" and rrank > 1:
        t[("rows", 0)] = "all"
        t[("cols", 0)] = "all"
    if name == TIE_CASE:
        t[("rows", TIE_ROUND - 1)] = "pair"      # (under 'origin' select[0] = -1 takes no argmax: select[j] is argmax j - 1)
    return t


def case(name, seed=None):
    """dict(data float32, rrank, metric, init, rid, cid, scores_r, scores_c, rid32, cid32, scores_r32, scores_c32, C, U, R, ferr,
    gram, twin): the float64 oracle of one SIVM_CUR.factorize() on the float32-representable data."""
    key = (name, seed)
    if key not in _cache:
        rows, cols, rrank, _, _, _, metric, init = _spec(name)
        d = data(name, seed)
        d64 = d.astype(np.float64)
        rid, sr = all_scores(d64.T, rrank, metric, init)
        cid, scs = all_scores(d64, rrank, metric, init)
        rid32, sr32 = all_scores(d64.T, rrank, metric, init, f32_dist=True)
        cid32, scs32 = all_scores(d64, rrank, metric, init, f32_dist=True)
        ones = np.ones(rrank)
        C, U, R = co.compute_ucr(d64, rid, ones, cid, ones)
        gram = co.gram_form(d64, rid, ones, cid, ones)
        _cache[key] = dict(data=d, rrank=rrank, metric=metric, init=init, rid=rid, cid=cid, scores_r=sr, scores_c=scs, rid32=rid32,
                           cid32=cid32, scores_r32=sr32, scores_c32=scs32, C=C, U=U, R=R, ferr=co.ferr(d64, C, U, R), gram=gram,
                           twin=co.twin(d64, rid, ones, cid, ones))
    return _cache[key]


def rel_max(a, b):
    """max |a - b| relative to max |b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def u_deviation(c):
    return rel_max(c["twin"]["U"], c["U"])


def twin_ferr(c):
    """The error of the float32 twin with the residual pass as the device runs it (k_resid, pmf_tiled.h): W = float32(C U) and
    H = float32(R) multiplied and subtracted from the data in float32, as cur_oracle.twin does, and then -- what that twin
    leaves out -- the squares formed in float32 and the 16 entries a lane holds (4 rows x 4 columns) summed in float32 before
    anything is float64.  On large data the two twins agree; on the six entries of the docstring case cur_oracle.twin's
    float32 arithmetic happens to be exact (deviation 7e-16) and the float32 squares are all the rounding there is."""
    d = c["data"]
    W = np.dot(c["twin"]["C"], c["twin"]["U"]).astype(np.float32)
    r = d - np.dot(W, c["twin"]["R"].astype(np.float32))
    m, n = r.shape
    sq = np.zeros(((m + 3) // 4 * 4, (n + 3) // 4 * 4), dtype=np.float32)
    sq[:m, :n] = r * r
    lanes = sq.reshape(sq.shape[0] // 4, 4, sq.shape[1] // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16)
    acc = np.zeros(lanes.shape[0], dtype=np.float32)
    for t in range(16):
        acc = (acc + lanes[:, t]).astype(np.float32)
    return float(np.sqrt(acc.astype(np.float64).sum()))


def ferr_deviation(c):
    """|ferr(twin) - ferr(oracle)| relative to ||data||, the larger of cur_oracle.twin's and twin_ferr's."""
    nrm = float(np.linalg.norm(c["data"].astype(np.float64)))
    return max(abs(c["twin"]["ferr"] - c["ferr"]), abs(twin_ferr(c) - c["ferr"])) / nrm


def well_posed(name, c):
    """None, or what keeps the case from being well posed: the gaps (ties by construction held to what they are), the float32
    selections, the spectrum condition of tests/test_cur_cases.py."""
    ties = expected_ties(name)
    for side, sel, s64, s32 in (("rows", c["rid"], c["scores_r"], c["scores_r32"]), ("cols", c["cid"], c["scores_c"], c["scores_c32"])):
        for tag, scores in (("f64", s64), ("f32", s32)):
            for j, (g2, g3) in enumerate(gaps(scores, sel, c["init"])):
                kind = ties.get((side, j))
                if kind == "all":
                    if not np.all(scores[j] == scores[j][0]):
                        return "%s %s argmax %d: not the all-equal tie" % (side, tag, j)
                elif kind == "pair":
                    if g2 != 0.0 or g3 < sc.MIN_GAP:
                        return "%s %s argmax %d: tie gaps %.2e %.2e" % (side, tag, j, g2, g3)
                elif g2 < sc.MIN_GAP:
                    return "%s %s argmax %d: gap %.2e" % (side, tag, j, g2)
    if c["rid32"] != c["rid"] or c["cid32"] != c["cid"]:
        return "float32 distances select other indices"
    g = c["gram"]
    kept = np.concatenate([g["kept_c"], g["kept_r"]])
    dropped = np.concatenate([g["dropped_c"], g["dropped_r"], [0.0]])
    s2 = max(1.0, _spec(name)[4]) ** 2           # the kept bounds follow the squared scale of shifted data; svd.py's cut does not
    if name != "doc_2x3" and not (kept.min() >= 1e-3 * s2 and np.abs(dropped).max() <= 1e-10 and kept.max() <= 1e6 * s2):
        return "spectrum: kept [%.2e, %.2e], dropped <= %.2e" % (kept.min(), kept.max(), np.abs(dropped).max())
    return None


def device_tol_u():
    return FACTOR * TWIN_U_DEV


def device_tol_ferr():
    return FACTOR * TWIN_FERR_DEV


def search():
    """Repeat the seed search and print the seeds and the twin deviations."""
    worst_u, worst_f = (0.0, None), (0.0, None)
    for name in list(CASES) + list(GOLDEN_ONLY):
        seed = None
        if name != "doc_2x3":
            for seed in range(SEARCH_FROM[name], SEARCH_FROM[name] + 400):
                why = well_posed(name, case(name, seed))
                if why is None:
                    break
                print("  %s seed %d: %s" % (name, seed, why))
            else:
                raise SystemExit("no seed for " + name)
        c = case(name, seed)
        du, df = u_deviation(c), ferr_deviation(c)
        print("%s: seed %s rid %s cid %s U deviation %.3e ferr deviation %.3e" % (name, seed, c["rid"][:8], c["cid"][:8], du, df))
        worst_u, worst_f = max(worst_u, (du, name)), max(worst_f, (df, name))
    print("worst U %.3e (%s), worst ferr %.3e (%s)" % (worst_u + worst_f))


if __name__ == "__main__":
    search()
