"""pymf_amd.CURSL without a GPU: the export, the constructor attributes, the refusals, and the leverage kernels in the built
library."""
import os
import re
import sys

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])


def test_export_is_declared_bound_and_documented():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_cur_leverage\(pmf_ctx\*\s*ctx,\s*int32_t k_rows,\s*int32_t k_cols,\s*double\*\s*row_lev,\s*"
                     r"double\*\s*col_lev\);", header)
    assert re.search(r"^ \*   pmf_cur_leverage\s+CURSL\.sample_probability", header, flags=re.M)
    assert "pmf_cur_leverage" in [s[0] for s in _lib.SYMBOLS]
    assert callable(_lib.Context.cur_leverage)
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        assert "CURSL" in text and ("pmf_cur_leverage" in text or doc == "README.md"), doc
    assert "CURSL" in pymf_amd.__all__
    assert issubclass(pymf_amd.CURSL, pymf_amd.CMD) and pymf_amd.CURSL is pymf_amd.cursl.CURSL


def test_constructor_attributes():
    mdl = pymf_amd.CURSL(DOC, rrank=1, crank=2)
    # cursl.py:63 hands crank=rrank to SVD.__init__: the crank argument is ignored
    assert (mdl._rows, mdl._cols, mdl._rrank, mdl._crank, mdl._k) == (2, 3, 1, 1, -1)
    assert mdl.data is DOC and pymf_amd.CURSL._EPS == 1e-8
    mdl = pymf_amd.CURSL(DOC)                                  # rrank = 0: all rows, all columns
    assert (mdl._rrank, mdl._crank) == (2, 3)
    with pytest.raises(AttributeError):
        mdl.frobenius_norm()                                   # no U yet, as in the reference
    for name in ("sample", "sample_probability", "computeUCR", "factorize", "_cmdinit"):
        assert callable(getattr(mdl, name))
    assert pymf_amd.CURSL.factorize is pymf_amd.CMD.factorize and pymf_amd.CURSL.computeUCR is pymf_amd.CUR.computeUCR
    assert pymf_amd.CURSL.sample_probability is not pymf_amd.CUR.sample_probability


def test_refusals(monkeypatch):
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(TypeError):
        pymf_amd.CURSL(sp.csr_matrix(np.ones((3, 5))), rrank=2).factorize()
    with pytest.raises(ValueError):
        pymf_amd.CURSL(np.ones((200, 300), dtype=np.float32), rrank=129).factorize()
    with pytest.raises(ValueError):
        pymf_amd.CURSL(np.ones((200, 300), dtype=np.float32)).factorize()          # rrank = 0: 200 rows, 300 columns
    with pytest.raises(ValueError):
        pymf_amd.CURSL(np.ones((2433, 2433), dtype=np.float32), rrank=4).factorize()   # min(rows, cols) > 2432
    with pytest.raises(ValueError):
        pymf_amd.CURSL(np.ones((2433, 2433), dtype=np.float32), rrank=4).sample_probability()

    class World(object):
        size, rank, local_rank = 2, 0, 0

    monkeypatch.setattr(pymf_amd.dist, "world", lambda: World())
    with pytest.raises(NotImplementedError):
        pymf_amd.CURSL(np.ones((3, 5), dtype=np.float32), rrank=2).factorize()


def test_leverage_kernels_are_in_the_built_library():
    """Both orientations of k_lev_f64, every operand-tile count, without a private segment; the LDS a piece of the operand takes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf of the ROCm image is not here")
    rows = {r["dem"]: r for r in kernel_regs.kernels(_lib.LIB_PATH)}
    for trans in ("false", "true"):
        assert any(name.startswith("k_lev_f64<%s" % trans) for name in rows), trans
        for nt in range(1, 9):
            r = rows["k_lev_f64<%s, %d>" % (trans, nt)]
            assert int(r["scratch"]) == 0 and int(r["lds"]) == nt * 8192 and int(r["wg"]) == 256, r
            assert int(r["vgpr"]) <= (512 if nt > 4 else 256 if nt > 2 else 168), r      # one, two, three waves per SIMD
        assert "k_lev_gather<%s>" % trans in rows
    assert "k_lev_eig" in rows
