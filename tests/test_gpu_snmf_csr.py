"""SNMF on CSR data on the MI355X: every reachable form of the kernels of pmf_csr.h on the structures of
tests/snmf_csr_cases.py, through the C ABI (_lib.Context), against the float64 reference of the same step.

W = V M is held to a componentwise bound derived from the arithmetic (snmf_csr_cases.w_bound: M rounded once to float32, at
most L_r float32 multiply-adds on a row of L_r entries, one ulp of the result); rows without entries must be exactly 0.0.
H is held to the project's figures for these paths: 2e-5 (relative, Frobenius) behind the float32 (P | S) of a pass over
the rows, 2e-6 for the float64 H of the Gram-space loop.  Which kernel ran is read from pmf_kernel_stats.

PMF_WRITE_PARITY=<path> writes the worst ratios per form (the committed copy: profiles/snmf_csr_parity.json)."""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import snmf_csr_cases as sc
from conftest import rel_fro
from oracle.snmf_oracle import snmf_update_h
from pymf_amd import _lib

pytestmark = pytest.mark.gpu

H_TOL_PASS = 2e-5       # test_snmf_gram_space_loop_equals_pass_per_iteration: H behind a float32 (P | S), well-conditioned data
H_TOL_GRAM = 2e-6       # test_csr_snmf_is_reproducible_run_to_run: the float64 H of the Gram-space loop
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def achieved_errors():
    yield
    if _worst and os.environ.get("PMF_WRITE_PARITY"):
        with open(os.environ["PMF_WRITE_PARITY"], "w") as f:
            json.dump(dict(bound_w_ratio=1.0, tolerance_h_pass=H_TOL_PASS, tolerance_h_gram=H_TOL_GRAM, worst=_worst), f,
                      indent=1, sort_keys=True)


def note(form, what, value):
    slot = _worst.setdefault(form, {})
    slot[what] = max(slot.get(what, 0.0), float(value))


@functools.lru_cache(maxsize=None)
def cus():
    """The card's CU count from torch.cuda.get_device_properties -- asked in a child process, as tests/test_gpu_coop_tiles.py
    does: torch ships a HIP runtime of its own, and a process that holds it beside the one libpymf_hip.so is linked to aborts
    at exit (double free)."""
    out = subprocess.run([sys.executable, "-c",
                          "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "torch" not in sys.modules
    return int(out.stdout.split()[-1])


VARIANTS = {"dup": lambda c: sc.with_duplicates(c, 3), "shuffled": lambda c: sc.shuffled_rows(c, seed=5)}


@functools.lru_cache(maxsize=64)
def arrays(entry, n):
    """The CSR arrays of an atlas entry, "<entry>+dup" / "<entry>+shuffled" for its variants."""
    name, _, var = entry.partition("+")
    csr = sc.build(name, n, cus())
    return VARIANTS[var](csr) if var else csr


@functools.lru_cache(maxsize=16)
def first_step(entry, n, k):
    """(M, W, H) of one reference iteration from h0(n, k): shared by the tests of one (entry, n, k), never written to.  The
    variants share the reference of their base entry: the same matrix, another order of summation."""
    out = sc.reference_step(arrays(entry.partition("+")[0], n), n, sc.h0(n, k))
    for a in out:
        a.setflags(write=False)
    return out


def context(entry, n, k, gram=None, profile=False):
    indptr, indices, data = arrays(entry, n)
    m = indptr.shape[0] - 1
    c = _lib.Context(_lib.ALGO_SNMF, m, n, k)
    c.set_v_csr(indptr, indices, data)
    c.set_w(np.zeros((m, k), dtype=np.float32))
    c.set_h(sc.h0(n, k))
    if gram is not None:
        c.set_option("snmf_gram", gram)
    if profile:
        c.profile_enable()
    return c


def check_w(form, entry, n, M, W, Wdev, what="W"):
    ratio = sc.w_ratio(arrays(entry, n), n, M, W, Wdev)
    print("%s %s n=%d %s: error / bound = %.3g" % (form, entry, n, what, ratio))
    note(form, "w_error_over_bound", ratio)
    assert ratio <= 1.0, (form, entry, what, ratio)


def check_h(form, entry, Href, Hdev, tol, what="H"):
    e = rel_fro(Hdev, Href, what="%s %s %s" % (form, entry, what))
    print("%s %s %s: rel_fro = %.3g (tolerance %.1g)" % (form, entry, what, float(e), tol))
    note(form, "h_rel_fro_pass" if tol == H_TOL_PASS else "h_rel_fro_gram", float(e))
    assert e < tol, (form, entry, what, float(e))


W_ENTRIES = sc.SMALL + ("deep", "blocks16+dup", "blocks16+shuffled", "edge_tile+dup")


@pytest.mark.parametrize("entry", W_ENTRIES)
@pytest.mark.parametrize("form", sc.W_FORMS, ids=lambda f: "%s-%s" % (f[0], "lds" if f[1] else "l2"))
def test_w_step(form, entry):
    """update_w() = k_csr_w_blocks<NT>, M in LDS or through L2, on every structure of the atlas."""
    name, lds, n, k = form
    M, W, _ = first_step(entry, n, k)
    c = context(entry, n, k)
    c.update_w()
    Wdev = c.get_w()
    c.close()
    check_w(name + ("/lds" if lds else "/l2"), entry, n, M, W, Wdev)
    if entry == "empty":
        assert not Wdev.any()


PASS_ENTRIES = sc.SMALL + ("deep", "blocks16+dup", "blocks16+shuffled")
TWO_ITERATIONS = ("blocks16", "deep", "blocks16+dup")


@pytest.mark.parametrize("entry", PASS_ENTRIES)
@pytest.mark.parametrize("form", sc.PASS_FORMS, ids=lambda f: "%s-n%d" % (f[0], f[1]))
def test_pass_per_iteration(form, entry):
    """factorize(1) with snmf_gram = 0: one launch of k_snmf_csr_mfma<NT,NTP> or k_snmf_csr_fused<NT> forms W, P = W^T V and
    S = W^T W; a second iteration on the entries with blocks of more than 64 entries shows the LDS tile and mask of the MFMA
    kernel restored across blocks and launches."""
    name, n, k = form
    M, W, H1 = first_step(entry, n, k)
    c = context(entry, n, k, gram=0, profile=True)
    _, done, _ = c.factorize(1, compute_err=False)
    assert done == 1
    Wdev, Hdev = c.get_w(), c.get_h64()
    st = c.kernel_stats()
    assert st["name"] == name and st["launches"] == 1, st
    check_w(name, entry, n, M, W, Wdev)
    if entry == "empty":
        assert not Wdev.any() and not Hdev.any()
    else:
        check_h(name, entry, H1, Hdev, H_TOL_PASS)
    if entry in TWO_ITERATIONS:
        M2, W2, H2 = sc.reference_step(arrays(entry, n), n, Hdev)      # from the H the device holds: the step alone is judged
        c.factorize(1, compute_err=False)
        assert c.kernel_stats()["launches"] == 2 and c.kernel_stats()["name"] == name
        check_w(name, entry, n, M2, W2, c.get_w(), what="W of the second iteration")
        check_h(name, entry, H2, c.get_h64(), H_TOL_PASS, what="H of the second iteration")
    c.close()


HOOK_FORMS = sc.P_FORMS + [("k_csr_p<1>", 96, 40), ("k_csr_p<2>", 128, 65)]     # the last two: a one-pass kernel runs in factorize()
HOOK_ENTRIES = ("blocks16", "edge_col0", "edge_collast", "edge_tile", "blocks16+dup")


@pytest.mark.parametrize("entry", HOOK_ENTRIES)
@pytest.mark.parametrize("form", HOOK_FORMS, ids=lambda f: "%s-n%d" % (f[0], f[1]))
def test_hooks(form, entry):
    """update_w(); update_h() = k_csr_w_blocks, then W^T W and k_csr_p<VPL>: on a fresh context, and behind a pass-per-iteration
    factorize() -- first the H step alone (the (P | S) that factorize() left), then both hooks ((P | S) formed again)."""
    name, n, k = form
    assert sc.dispatch(n, k)["p"] == name
    csr = arrays(entry, n)
    V = sc.as_scipy(csr, n)
    M, W, H1 = first_step(entry, n, k)
    c = context(entry, n, k)
    c.update_w(); c.update_h()
    check_w(name, entry, n, M, W, c.get_w(), what="W of update_w")
    check_h(name, entry, H1, c.get_h64(), H_TOL_PASS, what="H of update_w; update_h")
    c.close()
    c = context(entry, n, k, gram=0)
    c.factorize(1, compute_err=False)
    Hd1 = c.get_h64()
    check_w(name, entry, n, M, W, c.get_w(), what="W of factorize")
    check_h(name, entry, H1, Hd1, H_TOL_PASS, what="H of factorize")
    c.update_h()                                                       # same W, the (P | S) at hand
    Hd2 = c.get_h64()
    check_h(name, entry, snmf_update_h(V, np.array(W), Hd1.copy()), Hd2, H_TOL_PASS, what="H of update_h on the kept (P | S)")
    M3, W3, H3 = sc.reference_step(csr, n, Hd2)
    c.update_w(); c.update_h()
    check_w(name, entry, n, M3, W3, c.get_w(), what="W of the hooks behind factorize")
    check_h(name, entry, H3, c.get_h64(), H_TOL_PASS, what="H of the hooks behind factorize")
    c.close()


GRAM_ENTRIES = ("gram_cap", "empty", "gram_cap+dup", "gram_cap+shuffled") + tuple("ragged_m%d" % m for m in sc.RAGGED_M)


GRAM_CASES = [(f, e) for f in sc.GRAM_FORMS for e in GRAM_ENTRIES] + [(f, "gram_deep") for f in sc.GRAM_FORMS if f[0] == "global"]


@pytest.mark.parametrize("form,entry", GRAM_CASES, ids=lambda v: v if isinstance(v, str) else "%s-n%d" % (v[0], v[1]))
def test_gram_space_iteration(form, entry):
    """factorize(1) with snmf_gram = 1: C = V^T V by k_csr_gram (images in LDS for np <= 128, in global memory beyond), exact
    fixed point -- two runs give the same bits -- and the float64 H behind it.  gram_deep: every wave passes seven blocks,
    staged and row-by-row forms in turn (built for the 256 waves of the global-image launch; the LDS form launches 2048)."""
    image, n, k = form
    assert sc.dispatch(n, k)["gram_image"] == image
    M, W, H1 = first_step(entry, n, k)
    runs = []
    for rep in range(2):
        c = context(entry, n, k, gram=1)
        _, done, _ = c.factorize(1, compute_err=False)
        assert done == 1
        Hd = np.empty((k, n))
        assert c.get_h_into(Hd)
        runs.append((c.get_w(), Hd))
        c.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    form_name = "k_csr_gram/" + image
    check_w(form_name, entry, n, M, W, runs[0][0])
    if entry == "empty":
        assert not runs[0][0].any() and not runs[0][1].any()
    else:
        check_h(form_name, entry, H1, runs[0][1], H_TOL_GRAM, what="float64 H")


def test_non_persistent_write():
    """k_csr_w_blocks with one workgroup per 256 rows and M through L2 (nwg_full >= 8 CUs): the launch form of the large sparse
    configuration of the benchmark."""
    n, k = 64, 16
    m = 8 * cus() * 256 + 16 * 3 + 5
    assert not sc.dispatch(n, k, m=m, cus=cus())["w_persistent"]
    lengths = np.random.RandomState(7).binomial(n, 0.005, size=m)
    csr = sc.csr_from_row_lengths(n, lengths, seed=8)
    H0 = sc.h0(n, k)
    Hf = H0.astype(np.float64)
    M = np.dot(Hf.T, np.linalg.inv(np.dot(Hf, Hf.T)))
    W = np.asarray(sc.as_scipy(csr, n) @ M)
    t0 = time.time()
    c = _lib.Context(_lib.ALGO_SNMF, m, n, k)
    c.set_v_csr(*csr)
    c.set_w(np.zeros((m, k), dtype=np.float32)); c.set_h(H0)
    c.update_w()
    Wdev = c.get_w()
    c.close()
    print("non-persistent write: m = %d, %.2f s on the device side" % (m, time.time() - t0))
    ratio = sc.w_ratio(csr, n, M, W, Wdev)
    print("k_csr_w_blocks<1>/non-persistent: error / bound = %.3g" % ratio)
    note("k_csr_w_blocks<1>/non-persistent", "w_error_over_bound", ratio)
    assert ratio <= 1.0


def test_malformed_uploads_are_refused_and_leave_the_data_alone():
    """pmf_set_v_csr_f32 on an SNMF context checks the arrays on the host: a refused upload never reaches the device, so the
    first upload's W comes out again.  No update follows an upload that was not refused."""
    n, k = 50, 7
    indptr, indices, data = arrays("blocks16", n)
    m = indptr.shape[0] - 1
    c = context("blocks16", n, k)
    c.update_w()
    W1 = c.get_w()
    bad = []
    ip = indptr.copy(); ip[0] = 1; bad.append((ip, indices, "indptr\\[0\\] must be 0"))
    ip = indptr.copy(); ip[-1] -= 1; bad.append((ip, indices, "indptr\\[m\\] must be nnz"))
    ip = indptr.copy(); ip[40], ip[41] = ip[41] + 1, ip[40]; bad.append((ip, indices, "indptr must not decrease"))
    for where, value in ((5, n), (0, -1), (len(indices) - 1, 63), (7, 2 ** 31 - 1), (9, 64)):
        ix = indices.copy(); ix[where] = value
        bad.append((indptr, ix, "column index out of range"))
    for ip, ix, why in bad:
        refused = False
        try:
            c.set_v_csr(ip, ix, data)
        except _lib.PmfError as e:
            refused = e.code == _lib.PMF_EINVAL
            assert "pmf_set_v_csr_f32: " in str(e) and __import__("re").search(why, str(e)), str(e)
        assert refused, why                                            # (an accepted upload ends the test here: nothing runs on it)
        c.update_w()
        assert np.array_equal(c.get_w(), W1), why
    c.close()
