"""tests/snmf_csr_cases.py held to the sources and to SciPy, without a GPU: the builders, the structures the atlas claims, the
dispatch model against pmf_host_snmf.h, a case for every reachable form, the two dead forms, and the reference."""
import numpy as np
import pytest
import scipy.sparse as sp

import snmf_csr_cases as sc
from oracle import SNMFOracle

ALL_N = sorted({f[2] for f in sc.reachable()})


@pytest.mark.parametrize("cols", ["random", "first", "last", "tile:1"])
def test_builder_rows_are_canonical(cols):
    n = 50
    lengths = [0, 1, 16, 5, 0, 16, 3] if cols.startswith("tile") else [0, 1, 50, 7, 0, 49, 13]
    indptr, indices, data = sc.csr_from_row_lengths(n, lengths, seed=3, cols=cols)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert np.array_equal(np.diff(indptr), lengths)
    for r in range(len(lengths)):
        c = indices[indptr[r]:indptr[r + 1]]
        assert np.all(np.diff(c) > 0) and (c.size == 0 or (c[0] >= 0 and c[-1] < n))
    assert np.all(data != 0) and data.min() > -0.3 - 1e-6 and data.max() < 0.7 and (data < 0).any() and (data > 0).any()
    if cols == "first":
        assert indices[indptr[1]] == 0
    if cols == "last":
        assert indices[indptr[2] - 1] == n - 1
    if cols == "tile:1":
        assert indices.min() >= 16 and indices.max() < 32


def test_variants_keep_the_dense_image():
    csr = sc.build("blocks16", 50)
    ref = sc.as_scipy(csr, 50).toarray()
    dup = sc.with_duplicates(csr, 3)
    shf = sc.shuffled_rows(csr, seed=4)
    assert dup[1].shape[0] == csr[1].shape[0] + len(range(0, csr[1].shape[0], 3))
    assert not sc.as_scipy(dup, 50).has_canonical_format
    assert any(np.any(np.diff(shf[1][shf[0][r]:shf[0][r + 1]]) < 0) for r in range(len(shf[0]) - 1))
    assert np.array_equal(sc.as_scipy(dup, 50).toarray(), ref)          # halves are exact: the same to the last bit
    assert np.array_equal(sc.as_scipy(shf, 50).toarray(), ref)
    assert np.array_equal(sp.csr_matrix((dup[2], dup[1], dup[0]), shape=ref.shape).toarray().astype(np.float64), ref)


@pytest.mark.parametrize("n", ALL_N)
def test_atlas_realises_its_structures(n):
    a = sc.atlas(n)
    b16 = sc.block16_counts(sc.build("blocks16", n)[0])
    assert list(b16[:9]) == list(sc.BLOCKS16_COUNTS) and list(b16[9:]) == list(sc.BLOCKS16_COUNTS)
    assert sorted(set(sc.BLOCKS16_COUNTS)) == [0, 1, 63, 64, 65, 127, 128, 129, 200]
    L = np.asarray(a["blocks16"][0]).reshape(18, 16)
    assert L[:9].max() <= 13 and np.all(L[2:9].min(axis=1) >= 3)       # spread: every row of the block holds entries
    assert all((L[9 + q] > 0).sum() == -(-c // n) for q, c in enumerate(sc.BLOCKS16_COUNTS))   # packed: as few rows as n allows
    assert (L[9:, 0] == 0).all() and (L[9:, 15] == 0).any() and (L[9:, 15] > 0).any()
    g = sc.block64_counts(sc.build("gram_cap", n)[0])
    assert list(g[:11]) == [0, 255, 256, 257, 40, 300, 400, 10, 0, 256, 100]
    staged = [t < sc.GRAM_CAP for t in g[4:11]]
    assert staged == [True, False, False, True, True, False, True]     # short long long short empty long short
    if n >= 255:
        assert g[11] == 255 and np.diff(sc.build("gram_cap", n)[0]).max() == 255
    else:
        assert len(g) == 11                                             # SKIPPED: a 255-entry row needs n >= 255
    for m in sc.RAGGED_M:
        ip = sc.build("ragged_m%d" % m, n)[0]
        assert ip.shape[0] == m + 1 and 0 < ip[-1] <= 4 * m
    assert sc.build("empty", n)[0].tolist() == [0] * 101
    assert set(sc.build("edge_col0", n)[1].tolist()) == {0} and set(sc.build("edge_collast", n)[1].tolist()) == {n - 1}
    t = sc.build("edge_tile", n)[1]
    assert t.min() // 16 == t.max() // 16 and t.max() - t.min() >= 12 and (t.max() // 16 + 1) * 16 <= n
    assert set(sc.atlas(n)) == set(sc.SMALL) | {"deep"}


@pytest.mark.parametrize("cus", [256, 304, 64])
@pytest.mark.parametrize("n", [50, 192, 1100])
def test_deep_passes_three_blocks_per_wave_with_a_remainder(n, cus):
    lengths = sc.deep_lengths(n, cus)
    m = len(lengths)
    wgs, per, extra = sc.pass_geometry(m, n, cus)
    assert per >= 3 and extra != 0 and m % 16 != 0 and wgs <= cus
    assert list(lengths[:288]) == sc.blocks16_lengths(n)
    assert 0.008 < lengths[288:].sum() / float((m - 288) * n) < 0.012
    # the head's blocks of more than 64 entries follow each other inside one wave's range
    b16 = sc.block16_counts(np.concatenate([[0], np.cumsum(lengths)]))
    assert per >= 3 and (b16[per:2 * per + 1] > 64).sum() >= 2


def test_gram_deep_gives_every_wave_the_whole_pattern():
    n = 255
    assert sc.gram_wgs(n) == 32 and sc.gram_wgs(128) == 256 and sc.gram_wgs(129) == 32
    g = sc.block64_counts(sc.build("gram_deep", n)[0])
    waves = 32 * sc.GRAM_WAVES
    assert len(g) == 7 * waves and len(g) % waves == 0                  # per = 7, extra = 0: wave w starts at block 7 w
    assert all(list(g[7 * w:7 * w + 7]) == list(sc.GRAM_DEEP_PATTERN) for w in range(waves))


def test_the_model_lists_the_switch_of_csr_mfma():
    assert sorted(sc.mfma_table()) == sorted(sc.MFMA_TABLE)
    covered = sorted(name for kind, name, n, k in sc.reachable() if name.startswith("k_snmf_csr_mfma"))
    assert covered == sorted("k_snmf_csr_mfma<%d,%d>" % t for t in sc.mfma_table())     # a new case cannot go untested


def test_every_reachable_form_has_a_case_that_dispatches_to_it():
    seen = set()
    for kind, name, n, k in sc.reachable():
        d = sc.dispatch(n, k)
        assert k <= n and not d["dense"], (name, n, k)
        if kind == "pass":
            assert d["pass"] == name and not d.get("one_region")
        elif kind == "p":
            assert d["p"] == name and d["pass"] is None                 # factorize(snmf_gram = 0) runs the hooks there
        elif kind == "w":
            assert d["w"] + ("/lds" if d["w_m_in_lds"] else "/l2") == name
        else:
            assert d["gram"] and d["gram_image"] == name
        seen.add((kind, name))
    # every form any solvable (n, k) reaches is among them
    want = set()
    for n in list(range(1, 2700, 7)) + [64, 128, 192, 320, 1216]:
        for k in (1, 7, 16, 17, 32, 33, 64, 65, 100, 128):
            d = sc.dispatch(n, k)
            if k > n or d["dense"]:
                continue
            if d["pass"]:
                want.add(("pass", d["pass"]))
            want.add(("p", d["p"]))
            want.add(("w", d["w"] + ("/lds" if d["w_m_in_lds"] else "/l2")))
            if d["gram"]:
                want.add(("gram", d["gram_image"]))
    assert want == seen, (want - seen, seen - want)
    assert sc.dispatch(1100, 5)["pass"] == "k_snmf_csr_fused<1>" and not sc.dispatch(1100, 5)["gram"]   # the default path there
    assert sc.dispatch(1216, 16)["pass"] == "k_snmf_csr_fused<1>" and sc.dispatch(1217, 16)["dense"] is False
    m_np = 8 * sc.MI355X_CUS * 256 + 16 * 3 + 5
    assert not sc.dispatch(64, 16, m=m_np)["w_persistent"] and sc.dispatch(64, 16, m=m_np - 512)["w_persistent"]


def test_the_dead_forms_are_dead():
    """k_snmf_csr_fused<8> needs NT = 8 at np = 64 (np = 128 is k_snmf_csr_mfma<8,8>, np >= 192 exceeds the LDS): more than 64
    bases on at most 64 columns.  The one-region S exchange needs 2 NS KiB > 4 np KP bytes: NT = 4 at np = 64 or NT = 8 at
    np = 128 (both the MFMA kernel's), or NT = 8 at np = 64 again.  With num_bases <= n neither is reached."""
    assert sc.dead_forms() == []
    assert sc.dispatch(64, 65)["pass"] == "k_snmf_csr_fused<8>" and sc.dispatch(64, 65)["one_region"]   # the ill-posed call
    for nt, kp in ((1, 16), (2, 32), (4, 64), (8, 128)):
        ns = nt * (nt + 1) // 2
        small = [npad for npad in range(64, 1280, 64) if 2 * ns * 1024 > npad * kp * 4]
        assert small == {1: [], 2: [], 4: [64], 8: [64, 128]}[nt]
        assert all((nt, npad // 16) in sc.MFMA_TABLE or (nt, npad) == (8, 64) for npad in small)


@pytest.mark.parametrize("kind,name,n,k", sc.reachable())
def test_h0_is_well_conditioned(kind, name, n, k):
    H = sc.h0(n, k).astype(np.float64)
    assert np.linalg.cond(H.dot(H.T)) < 1e6


def test_reference_equals_the_oracle_on_toarray_and_ignores_storage_order():
    n, k = 50, 7
    csr = sc.build("blocks16", n)
    H = sc.h0(n, k)
    M, W, H1 = sc.reference_step(csr, n, H)
    o = SNMFOracle(sc.as_scipy(csr, n).toarray(), num_bases=k)
    o.W, o.H = np.zeros((len(csr[0]) - 1, k)), H.astype(np.float64)
    o.update_w(); o.update_h()
    assert np.abs(W - o.W).max() <= 1e-12 * np.abs(o.W).max() and np.abs(H1 - o.H).max() <= 1e-11 * np.abs(o.H).max()
    for var in (sc.with_duplicates(csr, 3), sc.shuffled_rows(csr)):
        _, W2, H2 = sc.reference_step(var, n, H)
        assert np.abs(W2 - W).max() <= 1e-13 * np.abs(W).max() and np.abs(H2 - H1).max() <= 1e-12 * np.abs(H1).max()
        o2 = SNMFOracle(sc.as_scipy(var, n).toarray(), num_bases=k)     # the oracle itself on the variant's dense image
        o2.W, o2.H = o.W * 0, H.astype(np.float64)
        o2.update_w(); o2.update_h()
        assert np.array_equal(o2.W, o.W) and np.array_equal(o2.H, o.H)


def test_w_bound_accepts_float32_summation_and_refuses_a_lost_entry():
    n, k = 100, 16
    csr = sc.build("blocks16", n)
    M, W, _ = sc.reference_step(csr, n, sc.h0(n, k))
    M32 = M.astype(np.float32)
    indptr, indices, data = csr
    Wf = np.zeros(W.shape, dtype=np.float32)
    for r in range(W.shape[0]):                                          # the kernel's order: entry by entry, float32
        for e in range(indptr[r], indptr[r + 1]):
            Wf[r] = Wf[r] + data[e] * M32[indices[e]]
    assert sc.w_ratio(csr, n, M, W, Wf) <= 1.0
    for var in (sc.with_duplicates(csr, 3), sc.shuffled_rows(csr)):
        assert sc.w_ratio(var, n, M, W, Wf) <= 1.0
    r = int(np.argmax(np.diff(indptr)))
    bad = Wf.copy()
    bad[r] -= data[indptr[r] + 64 if indptr[r + 1] - indptr[r] > 64 else indptr[r]] * M32[indices[indptr[r]]]
    assert sc.w_ratio(csr, n, M, W, bad) > 10.0                          # one entry dropped or misread
    bad = Wf.copy()
    bad[np.diff(indptr) == 0] = 1e-30
    with pytest.raises(AssertionError, match="exactly zero"):
        sc.w_ratio(csr, n, M, W, bad)
