"""The shared cases of tests/sub_cases.py, checked on the CPU: the index patterns are what their names say, the special values
are in the data, and every 'cur' seed keeps its draws clear of the cumulative boundaries."""
import numpy as np
import pytest

import sub_cases as sc


def test_the_grid_is_the_issues():
    assert sc.ROWS == (1, 29, 64, 65, 300) and sc.SRC_COLS == (3, 300, 5000) and sc.NSEL == (1, 3, 16, 17, 64, 65, 130)
    assert sc.PATTERNS == ("ascending", "descending", "random_repeats", "one_column", "ends")
    # the extra widths sit on both sides of the two thresholds of the tiling (np = 256 and np = 1024 destination columns)
    np_of = lambda nsel: (nsel + 63) // 64 * 64
    assert [np_of(x) for x in sc.NSEL_EXTRA] == [256, 320, 1024, 1088]


@pytest.mark.parametrize("n", sc.SRC_COLS)
def test_index_patterns(n):
    for nsel, pattern, idx in sc.gather_cases(29, n):
        assert idx.dtype == np.int64 and idx.shape == (nsel,) and idx.min() >= 0 and idx.max() < n, (nsel, pattern)
        d = np.diff(idx)
        if pattern == "ascending":
            assert np.all(d > 0) if nsel <= n else np.all(d >= 0)
        elif pattern == "descending":
            assert np.all(d < 0) if nsel <= n else np.all(d <= 0)
        elif pattern == "random_repeats":
            assert nsel < 2 or np.unique(idx).shape[0] < nsel
        elif pattern == "one_column":
            assert np.all(idx == idx[0])
        else:
            assert (n - 1) in idx and (nsel < 2 or 0 in idx)
    # the same arguments give the same indices
    assert np.array_equal(sc.gather_index("random_repeats", n, 65), sc.gather_index("random_repeats", n, 65))


@pytest.mark.parametrize("rows", sc.ROWS)
@pytest.mark.parametrize("n", sc.SRC_COLS)
def test_data_hold_the_special_values(rows, n):
    V = sc.gather_data(rows, n)
    assert V.dtype == np.float32 and V.shape == (rows, n) and V.flags.c_contiguous
    bits = set(int(b) for b in V.view(np.uint32).reshape(-1))
    want = [int(b) for b in sc.SPECIALS]
    present = [b for b in want if b in bits]
    assert present                                             # (1 x 3: three places for seven values)
    if rows * n >= 64:
        assert present == want
        nan_bits = [b for b in want if np.isnan(np.uint32(b).view(np.float32))]
        assert len(set(nan_bits)) == 4                          # distinct payloads
    assert np.array_equal(V.view(np.uint32), sc.gather_data(rows, n).view(np.uint32))


@pytest.mark.parametrize("rows,n,nsub,seed", sc.CUR_CASES)
def test_cur_seeds_keep_clear_of_the_boundaries(rows, n, nsub, seed):
    V = sc.sub_data(rows, n)
    idx, margin = sc.cur_reference(V, nsub, seed)
    print("cur case %dx%d nsub=%d seed=%d: smallest distance to a boundary %.3e" % (rows, n, nsub, seed, margin))
    assert margin > sc.CUR_MARGIN
    assert idx.shape == (nsub,) and np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < n
    # ... so the indices are those of any summation order: float32-accurate norms give them too
    d = V.astype(np.float64)
    pcol = np.add.reduce(d[::-1] ** 2, axis=0)                 # another order
    pcol /= pcol.sum()
    cum = np.cumsum(pcol)
    np.random.seed(seed)
    again = np.sort([np.searchsorted(cum, np.random.rand(), side="left") for _ in range(nsub)])
    assert np.array_equal(idx, again)


def test_sub_data_is_positive_float32():
    V = sc.sub_data(*sc.COMPOSITION_SHAPE)
    assert V.dtype == np.float32 and V.min() > 0 and np.all((V.astype(np.float64) ** 2).sum(axis=0) > 0)
