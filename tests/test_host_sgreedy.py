"""pymf_amd.SIVM_SGREEDY without a GPU: the class surface, the constructor it shares with SIVM, the ordering of `select`."""
import inspect

import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib
from pymf_amd import sivm_sgreedy as mod


def test_class_surface():
    assert pymf_amd.SIVM_SGREEDY is mod.SIVM_SGREEDY and "SIVM_SGREEDY" in pymf_amd.__all__
    assert issubclass(pymf_amd.SIVM_SGREEDY, pymf_amd.SIVM)
    assert not issubclass(pymf_amd.LAESA, pymf_amd.SIVM_SGREEDY)
    for hook in ("update_w", "update_h", "factorize", "frobenius_norm", "init_w", "init_h"):
        assert callable(getattr(pymf_amd.SIVM_SGREEDY, hook))
    assert pymf_amd.SIVM_SGREEDY._MAX_BASES == 64 and pymf_amd.SIVM_SGREEDY._ALGO == _lib.ALGO_SIVM
    assert "pmf_sivm_get_volumes" in {s[0] for s in _lib.SYMBOLS}
    assert "not synchronised" in mod.__doc__ and "affinely independent" in mod.__doc__


def test_constructor_signature_is_sivms():
    assert inspect.signature(pymf_amd.SIVM_SGREEDY.__init__) == inspect.signature(pymf_amd.SIVM.__init__)
    assert inspect.signature(pymf_amd.SIVM_SGREEDY.factorize) == inspect.signature(pymf_amd.SIVM.factorize)
    mdl = pymf_amd.SIVM_SGREEDY(np.ones((3, 5)), num_bases=2, dist_measure="l1", init="origin")
    assert (mdl._num_bases, mdl._dist_measure, mdl._init) == (2, "l1", "origin")
    with pytest.raises(TypeError):
        pymf_amd.SIVM_SGREEDY(np.ones((3, 5)), num_bases=2, niter=10)      # (the reference's docstring, not its code)


def test_unsupported_arguments_raise_before_any_device_work():
    with pytest.raises(ValueError, match="num_bases > 64"):
        pymf_amd.SIVM_SGREEDY(np.ones((3, 80)), num_bases=65).update_w()
    with pytest.raises(NotImplementedError, match="kl"):
        pymf_amd.SIVM_SGREEDY(np.ones((3, 8)), num_bases=2, dist_measure="kl").update_w()
    with pytest.raises(ValueError, match="init"):
        pymf_amd.SIVM_SGREEDY(np.ones((3, 8)), num_bases=2, init="random").update_w()


def test_reference_order():
    assert mod.reference_order([7]) == [7]
    assert mod.reference_order([7, 3]) == [7, 3]
    assert mod.reference_order([7, 3, 9, 1]) == [3, 7, 9, 1]
    assert mod.reference_order([-1, 40, 5, 60]) == [-1, 5, 40, 60]
    assert mod.reference_order(np.array([3, 7, 9, 1], dtype=np.int32)) == [3, 7, 9, 1]      # idempotent, Python ints
    assert all(type(s) is int for s in mod.reference_order(np.array([4, 2, 8], dtype=np.int32)))
