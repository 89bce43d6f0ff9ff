"""The float64 NumPy CNMF oracle (tests/cnmf_oracle.py) against the reference's own results (tests/golden/cnmf_*.npz,
written by tests/golden/gen_golden_cnmf.py from pymf/cnmf.py and pymf/kmeans.py).  CPU only."""
import glob
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import cnmf_oracle

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "cnmf_*.npz")))


def reference_sel(seed, n, k):
    """kmeans.py:71 under random.seed(seed): random.sample over the sample indices."""
    random.seed(int(seed))
    return np.sort(random.sample(range(n), k))


def oracle_run(d):
    V = d["V"].astype(np.float64)
    k, niter = int(d["k"]), int(d["niter"])
    sel = reference_sel(d["random_seed"], V.shape[1], k)
    H, G, assigned = cnmf_oracle.cnmf_init(V, k, sel)
    W0 = d["W_user"] if "W_user" in d else None
    W, H, G, ferr = cnmf_oracle.cnmf_factorize(V, H, G, W=W0, niter=niter, compute_w=bool(d["compute_w"]),
                                               compute_h=bool(d["compute_h"]))
    return W, H, G, ferr, sel


def test_there_are_cnmf_goldens():
    assert len(CASES) >= 9, CASES


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference_golden(name):
    d = load_golden(name)
    W, H, G, ferr, sel = oracle_run(d)
    assert len(ferr) == len(d["ferr"])
    np.testing.assert_allclose(ferr, d["ferr"], rtol=1e-12, atol=0)
    for a, mine in (("H", H), ("G", G), ("W", W)):
        if a in d:
            ref = d[a]
            assert np.linalg.norm(mine - ref) <= 1e-12 * np.linalg.norm(ref), a


@pytest.mark.parametrize("name", CASES)
def test_golden_keeps_a_margin_between_centres(name):
    """Only seeds whose k-means never came within 1e-5 (relative) of a tie were kept: the oracle sees the same gap."""
    d = load_golden(name)
    V = d["V"].astype(np.float64)
    sel = reference_sel(d["random_seed"], V.shape[1], int(d["k"]))
    _, _, gap = cnmf_oracle.kmeans(V, int(d["k"]), sel)
    assert gap >= 1e-5
    assert abs(gap - float(d["min_gap"])) <= 1e-9 * max(1.0, gap)
