"""The SVD / PCA cases leave room for the comparison on the device (no GPU): by construction the kept eigenvalues are far above
svd.py's 1e-8 cut, the dropped ones far below, adjacent singular values 5 % apart, the float32 twin finds the oracle's rank,
and the twin's deviation from the oracle stays within the committed figures that the device tolerances are derived from."""
import os
import re

import numpy as np
import pytest

import svd_cases as sc
import svd_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_match_the_library():
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_svd.h")) as f:
        dev = f.read()
    assert int(re.search(r"PMF_SVD_MIN_CHUNK = (\d+);", dev).group(1)) == sc.MIN_CHUNK
    assert int(re.search(r"PMF_SVD_TARGET_WGS = (\d+);", dev).group(1)) == sc.TARGET_WGS
    assert int(re.search(r"PMF_SVD_MAX_RANK = (\d+);", dev).group(1)) == sc.MAX_RANK
    import pymf_amd.svd
    assert pymf_amd.svd.MAX_RANK == sc.MAX_RANK


def test_chunking_covers_one_chunk_and_a_ragged_tail():
    assert sc.chunks(320, 1) == (1, 320)                       # 300 columns or rows: one chunk
    assert sc.chunks(2112, 1) == (4, 576)                      # 2 100: four chunks, the last 384 long
    assert sc.chunks(2112, 6) == (4, 576)                      # the same under three tiles per side (130 -> 192)
    assert sc.chunks(1048576, 1) == (512, 2048)                # 64 x 1 048 576: a few hundred workgroups


def _conditions(data64, name):
    left, kept, _, allv = so.gram_eig(so.f32(data64))
    s = np.sqrt(kept)
    dropped = allv[allv <= so.EPS]
    print("%s rank %d  min kept %.3e (%.3e of the largest)  max dropped %.3e  min step %.4f" % (
        name, len(kept), kept.min(), kept.min() / kept.max(), dropped.max() if dropped.size else 0.0,
        (s[:-1] / s[1:]).min() if len(s) > 1 else np.inf))
    assert kept.min() > 1e-4 * kept.max() and kept.min() > 1e-6
    _, _, _, allv64 = so.gram_eig(np.asarray(data64, dtype=np.float64))
    assert np.all(allv64[allv64 <= so.EPS] < 1e-10) and np.all(dropped < 1e-10)
    assert len(s) < 2 or (s[:-1] / s[1:]).min() >= 1.05 - 1e-9
    return len(kept)


@pytest.mark.parametrize("name", sorted(sc.SVD_CASES))
def test_svd_case_is_well_posed(name):
    c = sc.svd_case(name)
    r = _conditions(c["data"].astype(np.float64), name)
    assert r == c["S"].shape[0] == so.svd(c["data"], f32_twin=True)[1].shape[0]


@pytest.mark.parametrize("name", sorted(sc.PCA_CASES))
def test_pca_case_is_well_posed(name):
    c = sc.pca_case(name)
    r = _conditions(c["oracle"]["data"], name)
    twin = so.pca(c["data"], c["num_bases"], c["center_mean"], f32_twin=True)
    assert twin["W"].shape == c["oracle"]["W"].shape
    assert c["oracle"]["W"].shape[1] == (min(c["num_bases"], r) if c["num_bases"] else r)


def test_centring_leaves_a_null_eigenvalue_that_is_dropped():
    c = sc.pca_case("300x40_centred")
    assert c["oracle"]["W"].shape == (300, 39)


def test_committed_tolerances_hold_the_twin():
    """tests/golden/svd_tolerances.json holds the oracle-vs-twin figures rounded up to two digits: a new measurement stays
    within them and has not fallen to less than half (the file would then be stale)."""
    committed, now = sc.tolerances(), sc.measure()
    print(now)
    assert set(committed) == set(sc.QUANTITIES)
    for q in sc.QUANTITIES:
        assert now[q] <= committed[q], q
        assert now[q] >= 0.5 * committed[q], q
