"""The host-only check of CSR arrays (pmf_check_csr) that both branches of pmf_set_v_csr_f32 run before anything is uploaded,
without a GPU: the export, the refusals with their messages, and what passes (repeated entries and unsorted rows included)."""
import os
import re

import numpy as np
import pytest

import snmf_csr_cases as sc
from pymf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_is_declared_bound_and_shared_by_both_branches():
    with open(os.path.join(ROOT, "include", "pymf_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+pmf_check_csr\(int64_t m, int64_t n, const int64_t\*\s*indptr, const int32_t\*\s*indices, int64_t nnz\);", header)
    assert "pmf_check_csr" in [s[0] for s in _lib.SYMBOLS] and callable(_lib.check_csr)
    _lib.load()
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_api.hip")) as f:
        api = f.read()
    with open(os.path.join(ROOT, "pymf_amd", "csrc", "pmf_host_nmf_csr.h")) as f:
        nmf = f.read()
    snmf_branch = api[api.index("int pmf_set_v_csr_f32("):api.index("int pmf_check_csr(")]
    assert snmf_branch.index("csr_check(") < snmf_branch.index("dgrow(")            # before the first device call
    nmf_branch = nmf[nmf.index("int nmf_csr_set_v("):]
    assert nmf_branch.index("csr_check(") < nmf_branch.index("dgrow(")
    assert len(re.findall(r"column index out of range", api + nmf)) == 1            # one function, one message


def test_the_host_check_of_the_arrays():
    m, n = 288, 50
    indptr, indices, _ = sc.build("blocks16", n)
    _lib.check_csr(m, n, indptr, indices)                                            # canonical arrays pass
    _lib.check_csr(3, 2, [0, 0, 0, 0], [])                                           # an empty matrix too
    for var in (sc.with_duplicates(sc.build("blocks16", n), 3), sc.shuffled_rows(sc.build("blocks16", n))):
        _lib.check_csr(m, n, var[0], var[1])                                         # repeated entries, unsorted rows
    _lib.check_csr(1, 3, [0, 4], [2, 2, 0, 2])

    def refused(ip, ix, why, m=m, n=n):
        with pytest.raises(_lib.PmfError, match="pmf_check_csr: .*" + why) as e:
            _lib.check_csr(m, n, ip, ix)
        assert e.value.code == _lib.PMF_EINVAL

    ip = indptr.copy(); ip[40], ip[41] = ip[41] + 1, ip[40]
    refused(ip, indices, "indptr must not decrease")
    ip = indptr.copy(); ip[-1] -= 1
    refused(ip, indices, "indptr\\[m\\] must be nnz")
    ip = indptr.copy(); ip[-1] += 1
    refused(ip, indices, "indptr\\[m\\] must be nnz")
    ip = indptr.copy(); ip[0] = 1
    refused(ip, indices, "indptr\\[0\\] must be 0")
    for where, value in ((5, n), (0, -1), (len(indices) - 1, 63), (7, 2 ** 31 - 1)):   # 63: inside the padding of 50 columns
        bad = indices.copy(); bad[where] = value
        refused(indptr, bad, "column index out of range")
    with pytest.raises(ValueError):
        _lib.check_csr(m + 1, n, indptr, indices)
    with pytest.raises(_lib.PmfError, match="bad arguments"):
        _lib.check_csr(0, 5, [0], [])
