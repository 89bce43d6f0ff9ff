"""No GPU: the cases of tests/test_gpu_coop_tiles.py are what tests/coop_cases.py says they are -- every instantiation
pmf_coop.h lists is reached by its two cases through the host's own shape rules, and at 256 CUs every workgroup of
every case passes a first, a middle and a last tile."""
import numpy as np
import pytest

import coop_cases as cc


def test_table_has_seven_shapes_and_eighteen_instantiations():
    table = cc.dispatch_table()
    shapes = [t[:3] for t in table]
    assert len(shapes) == 7 and len(set(shapes)) == 7
    inst = cc.instantiations()
    assert len(inst) == 18 and len(set(inst)) == 18
    assert sorted(s for s, modes in ((t[:3], t[3]) for t in table) if "rnmf" in modes) == [(2, 4, p) for p in (1, 2, 3, 4)]
    names = [cc.kernel_name(*i) for i in inst]
    assert len(set(names)) == 18
    assert "k_nmf_coop<2,4,4>" in names and "k_nmf_coop<1,4,8,bnmf>" in names and "k_nmf_coop<2,4,1,rnmf>" in names


def test_every_case_reaches_its_instantiation_through_the_host_rules():
    cases = cc.cases()
    assert len(cases) == 36 and len(set(c[0] for c in cases)) == 36
    for cid, name, shape, mode, kind, m, n, k in cases:
        assert cc.host_instantiation(mode, n, k) == shape, cid
        assert name == cc.kernel_name(*shape, mode)
    for inst in cc.instantiations():
        kinds = sorted(c[4] for c in cases if (c[2] + (c[3],)) == inst)
        assert kinds == ["full", "ragged"], inst
    # RNMF is dispatched on <2,4,*> alone: the other shapes' sizes go elsewhere under RNMF
    for bt, rb, pn, modes in cc.dispatch_table():
        if "rnmf" not in modes:
            assert cc.host_instantiation("rnmf", 64 * pn, 64 * bt) is None


def test_full_cases_have_no_padding_and_ragged_cases_have_all_three():
    for cid, name, (bt, rb, pn), mode, kind, m, n, k in cc.cases():
        if kind == "full":
            assert (m % 64, n, k) == (0, 64 * pn, 64 * bt), cid
        else:
            assert cc.round_up(m, 64) == cc.M_FULL and m - (cc.M_FULL - 64) == 7, cid
            assert n % 64 != 0 and n % 16 == 0, cid
            # a wave owns 16 BT bases: wave (k // (16 BT)) is cut by k, the last wave owns pad bases only
            assert k % (16 * bt) != 0 and k // (16 * bt) < 3, cid
    ragged_n = {c[2]: c[6] for c in cc.ragged_cases()}
    assert [ragged_n[(2, 4, p)] for p in (1, 2, 3, 4)] == [16, 80, 144, 208]
    assert (ragged_n[(2, 2, 6)], ragged_n[(1, 4, 6)], ragged_n[(1, 4, 8)]) == (272, 272, 400)
    # ... the lower end: 16 columns fewer and the host chooses another instantiation (or another kernel)
    for cid, name, shape, mode, kind, m, n, k in cc.ragged_cases():
        assert cc.host_instantiation(mode, n - 16, k) != shape, cid


def test_every_workgroup_has_a_first_a_middle_and_a_last_tile():
    assert cc.tiles(cc.M_FULL, 4) == (550, 256, 2, 38)
    assert cc.tiles(cc.M_FULL, 2) == (1100, 256, 4, 76)
    for cid, name, (bt, rb, pn), mode, kind, m, n, k in cc.cases():
        ntiles, wgs, per, extra = cc.tiles(m, rb)
        assert wgs == cc.CUS and per >= 2 and 0 < extra < wgs, cid
        assert ntiles >= 2 * cc.CUS + 1 and ntiles % cc.CUS != 0, cid      # what the device test asks of the real card


def test_tile_position_restates_the_kernels_deal():
    for rb in (4, 2):
        ntiles, wgs, per, extra = cc.tiles(cc.M_RAGGED, rb)
        seen = []
        for b in range(wgs):                          # k_nmf_coop: t0, ntile of block b
            t0 = b * per + (b if b < extra else extra)
            for tt in range(per + (1 if b < extra else 0)):
                seen.append(t0 + tt)
                assert cc.tile_position(t0 + tt, cc.M_RAGGED, rb) == (b, t0, tt, per + (1 if b < extra else 0))
        assert seen == list(range(ntiles))


def test_slices_run_one_tile_per_workgroup():
    for rb in (4, 2):
        ntiles, wgs, per, extra = cc.tiles(cc.SLICE_ROWS, rb)
        assert ntiles <= cc.CUS and (per, extra) == (1, 0)
    assert cc.SLICE_ROWS % 64 == 0                    # a slice starts on the lanes it has in the whole matrix


def test_only_the_widest_shape_has_dmas_left_behind_the_s_part():
    """The `for (dd_ = RB BT 4 2; dd_ < NDMA; ...)` loop of the S part: if the DMA counts are retuned, this says which
    shapes cover it."""
    left = [(bt, rb, pn) for bt, rb, pn, _ in cc.dispatch_table() if cc.dma_beside_s(bt, rb) < cc.ndma(bt, rb, pn)]
    assert left == [(1, 4, 8)]
    assert cc.ndma(1, 4, 8) == 36 and cc.dma_beside_s(1, 4) == 32


def test_inputs_are_seeded_float32_values():
    case = ("tiny", "k_nmf_coop<2,4,1,rnmf>", (2, 4, 1), "rnmf", "ragged", 700, 16, 67)
    V, W0, H0 = cc.inputs(case)
    V2, W2, H2 = cc.inputs(case)
    assert V.dtype == np.float32 and np.array_equal(V, V2) and np.array_equal(W0, W2) and np.array_equal(H0, H2)
    assert np.array_equal(W0, W0.astype(np.float32)) and np.array_equal(H0, H0.astype(np.float32))
    assert np.count_nonzero(V > 1.0) in range(30, 38)          # one entry in 300, less collisions
    Vb = cc.inputs(("tiny", "k_nmf_coop<2,4,1,bnmf>", (2, 4, 1), "bnmf", "ragged", 700, 16, 67))[0]
    assert set(np.unique(Vb)) == {0.0, 1.0} and abs(Vb.mean() - 0.3) < 0.02
    seeds = set()
    for c in cc.cases():
        bt, rb, pn = c[2]
        seeds.add(1000 * (100 * bt + 10 * rb + pn) + 10 * cc.MODES.index(c[3]) + (c[4] == "ragged"))
    assert len(seeds) == 36
