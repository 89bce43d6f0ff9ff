"""The one-pass kernel's results are fixed bit for bit: W and H after three iterations of every k_nmf_fused
instantiation the dispatch reaches equal the digests in tests/golden/fused_bits.json, recorded by
tools/record_fused_bits.py (fused_bits_cases.py has the shapes).  A change to the kernel that only reschedules work
leaves them alone; one that moves a single rounding does not."""
import json

import pytest

import fused_bits_cases as fb


def _fixture():
    with open(fb.FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_every_instantiation_of_the_dispatch_table():
    fx = _fixture()
    assert fx["niter"] == fb.NITER
    table = fb.dispatch_table()
    assert len(table) == 18 and len(set(table)) == 18, table      # 15 one-block-per-wave + 3 two-waves-per-block
    want = {cid: (name, mode, m, n, k) for cid, name, mode, m, n, k in fb.cases()}
    assert len(want) == 2 * (15 * 4 + 3 * 3)
    assert set(fx["cases"]) == set(want)
    for cid, c in fx["cases"].items():
        assert (c["kernel"], c["mode"], c["m"], c["n"], c["k"]) == want[cid], cid
        assert len(c["W"]) == 64 and len(c["H"]) == 64, cid


@pytest.mark.gpu
@pytest.mark.parametrize("case", fb.cases(), ids=[c[0] for c in fb.cases()])
def test_fused_bits_match_recorded_digests(case):
    from pymf_amd import _lib
    cid, name, mode, m, n, k = case
    want = _fixture()["cases"][cid]
    path, hw, hh = fb.run_case(_lib, mode, m, n, k)
    assert path == name
    assert (hw, hh) == (want["W"], want["H"]), "%s: W or H differs in bits from the recorded run" % cid
