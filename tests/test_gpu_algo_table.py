"""What the C ABI's entry points say per algorithm number: the path names, the refusals and their messages, and SIVM's W step
against the column-panel path of pmf_sivm_select.  Every expected string and count is the library's before its algorithms
moved into one table (pmf_host_algos.h), so the table cannot rename, reorder or drop one unnoticed."""
import numpy as np
import pytest

import sivm_cases as sc
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

M, N, K = 20, 70, 3

# algorithm number -> (base count of the 20 x 70 context, pmf_path_name)
PATHS = {
    _lib.ALGO_NMF: (K, "k_nmf_fused<1,2>"),
    _lib.ALGO_NMFALS: (K, "tiled"),
    _lib.ALGO_SNMF: (K, "k_nmf_fused<1,2,snmf>"),
    _lib.ALGO_BNMF: (K, "k_nmf_fused<1,2,bnmf>"),
    _lib.ALGO_RNMF: (K, "k_nmf_fused<1,2,rnmf>"),
    _lib.ALGO_CNMF: (K, "cnmf_gram"),
    _lib.ALGO_KMEANS: (K, "cluster_panels"),
    _lib.ALGO_CMEANS: (K, "cluster_panels"),
    _lib.ALGO_SIVM: (K, "sivm_panels"),
    _lib.ALGO_AA: (K, "aa_pricing"),
    _lib.ALGO_PCA: (M, "svd_gram_f64"),          # (the base count must reach min(rows, cols))
    _lib.ALGO_CUR: (K, "cur_cross_f64"),
    _lib.ALGO_GREEDY: (K, "greedy_panels"),
}
BAD_ALGO = ("algo must be 0 (NMF), 1 (NMFALS), 2 (SNMF), 3 (BNMF), 4 (RNMF), 5 (CNMF), 6 (Kmeans), 8 (Cmeans), 10 (SIVM), 11 (AA), "
            "12 (PCA / SVD), 14 (CUR / CMD) or 15 (GREEDY)")
NOT_STREAMED = (_lib.ALGO_RNMF, _lib.ALGO_CNMF, _lib.ALGO_KMEANS, _lib.ALGO_CMEANS, _lib.ALGO_SIVM, _lib.ALGO_AA, _lib.ALGO_PCA,
                _lib.ALGO_CUR, _lib.ALGO_GREEDY)
ONE_RANK = {
    _lib.ALGO_CNMF: "CNMF", _lib.ALGO_KMEANS: "Kmeans / Cmeans", _lib.ALGO_CMEANS: "Kmeans / Cmeans", _lib.ALGO_SIVM: "SIVM",
    _lib.ALGO_AA: "AA", _lib.ALGO_PCA: "PCA / SVD", _lib.ALGO_CUR: "CUR / CMD", _lib.ALGO_GREEDY: "GREEDY",
}
# (algo, m, n, k) -> the first limit of the family
LIMITS = [
    (_lib.ALGO_SIVM, M, N, 65, "SIVM: num_bases > 64 is not supported by this build"),
    (_lib.ALGO_AA, M, N, 65, "AA: num_bases > 64 is not supported by this build"),
    (_lib.ALGO_GREEDY, M, N, 65, "GREEDY: num_bases > 64 is not supported by this build"),
    (_lib.ALGO_CUR, M, N, 129, "CUR / CMD: more than 128 sampled rows or columns are not supported by this build"),
    (_lib.ALGO_CNMF, M, 4097, K, "CNMF: n (samples) > 4096 is not supported by this build"),
    (_lib.ALGO_KMEANS, M, N, 129, "Kmeans / Cmeans: num_bases > 128 is not supported by this build"),
    (_lib.ALGO_PCA, M, N, K, "PCA / SVD: the context's base count must be at least min(rows, cols) (the largest possible rank)"),
    # where two could fire, the family's own comes first
    (_lib.ALGO_SIVM, M, N, 3000, "SIVM: num_bases > 64 is not supported by this build"),
    (_lib.ALGO_NMFALS, M, N, 1025, "num_bases > 1024 is not supported for NMFALS / NMFNNLS by this build"),
    (_lib.ALGO_NMF, M, N, 2433, "num_bases > 2432 is not supported by this build"),
]


def refused(msg, fn, *args, **kw):
    """fn(*args) returns PMF_EINVAL and pmf_last_error is `msg`, byte for byte"""
    with pytest.raises(_lib.PmfError) as e:
        fn(*args, **kw)
    print(e.value)
    assert e.value.code == _lib.PMF_EINVAL
    assert str(e.value) == "libpymf_hip error -1: " + msg


def test_path_names():
    assert sorted(PATHS) == [0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 14, 15]
    for algo, (k, path) in sorted(PATHS.items()):
        ctx = _lib.Context(algo, M, N, k)
        try:
            print(algo, ctx.path_name)
            assert ctx.path_name == path
        finally:
            ctx.close()
    for algo in (7, 9, 13, -1, 16):
        refused(BAD_ALGO, _lib.Context, algo, M, N, K)


def test_refusals():
    ctx = _lib.Context(_lib.ALGO_CUR, M, N, K)
    try:
        refused("CUR / CMD: no W step (pmf_cur_compute is the decomposition)", ctx.update_w)
        refused("CUR / CMD: no H step (pmf_cur_compute is the decomposition)", ctx.update_h)
        refused("CUR / CMD: no iteration (pmf_cur_compute is the decomposition)", ctx.factorize, 1)
    finally:
        ctx.close()
    for algo in NOT_STREAMED:
        ctx = _lib.Context(algo, M, N, PATHS[algo][0])
        try:
            refused("pmf_stream_*: NMF, BNMF, SNMF and NMFALS contexts", ctx.stream_begin)
        finally:
            ctx.close()
    for algo, family in sorted(ONE_RANK.items()):
        refused(family + ": one rank only in this build", _lib.Context, algo, M, N, PATHS[algo][0], nranks=2)
    for algo, m, n, k, msg in LIMITS:
        refused(msg, _lib.Context, algo, m, n, k)


@pytest.mark.parametrize("init", (0, 1))
@pytest.mark.parametrize("metric", (0, 1, 2))
def test_sivm_update_w_is_path_1(metric, init):
    """pmf_update_w and the column-panel path of pmf_sivm_select are one routine: the same selection, and k + 2 ('fastmap':
    three distance passes, then k - 1 rounds; sivm.py:145-201) or k ('origin') launches of k_sivm_pass."""
    c = sc.case("8x65600_k3_l2")
    V, k = c["V"], c["k"]
    ctx = _lib.Context(_lib.ALGO_SIVM, V.shape[0], V.shape[1], k)
    try:
        ctx.set_v_dense(V)
        ctx.set_option("sivm_metric", metric)
        ctx.set_option("sivm_init", init)
        ctx.profile_enable(True)
        ctx.update_w()
        stats = ctx.kernel_stats()
        ctx.profile_enable(False)
        got = ctx.get_select().tolist()
        want = ctx.sivm_select(k, False, metric, init, path=1).tolist()
        print(metric, init, got, want, stats["name"], stats["launches"])
        assert got == want
        assert stats["launches"] == (k if init == 1 else k + 2)
        if (metric, init) == (0, 0):
            assert got == c["select"]
    finally:
        ctx.close()
