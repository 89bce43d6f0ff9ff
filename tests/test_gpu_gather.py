"""pmf_set_v_gather_f32 / pmf_get_v_dense_f32 on the device: every gather case of tests/sub_cases.py is an exact copy (compared
as uint32: a copy has no tolerance); a context filled by gather cannot be told from one filled by pmf_set_v_dense_f32 (NMF,
NMFALS, Kmeans and SIVM: W, H, ferr or select array_equal -- the project states these paths bit-identical from run to run); every
refusal gives PMF_EINVAL with its message and leaves dst's data as they were; the event ordering gives what explicit
synchronisation gives."""
import random

import numpy as np
import pytest

import pymf_amd
import sub_cases as sc
from pymf_amd import _lib

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def holder(V, algo=_lib.ALGO_CUR, k=1):
    ctx = _lib.Context(algo, V.shape[0], V.shape[1], k)
    ctx.set_v_dense(V)
    return ctx


# ---- exact copy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.SRC_COLS)
@pytest.mark.parametrize("rows", sc.ROWS)
def test_exact_copy(rows, n):
    V = sc.gather_data(rows, n)
    src = holder(V)
    assert np.array_equal(bits(src.get_v_dense()), bits(V))                 # the download itself
    dst = {}
    for nsel, pattern, idx in sc.gather_cases(rows, n):
        if nsel not in dst:
            dst[nsel] = _lib.Context(_lib.ALGO_CUR, rows, nsel, 1)
        dst[nsel].set_v_gather(src, idx)
        got = dst[nsel].get_v_dense()
        assert np.array_equal(bits(got), bits(V[:, idx])), (rows, n, nsel, pattern)
    whole = _lib.Context(_lib.ALGO_CUR, rows, n, 1)
    whole.set_v_gather(src)                                                 # idx NULL: all columns in order
    assert np.array_equal(bits(whole.get_v_dense()), bits(V))
    assert np.array_equal(bits(src.get_v_dense()), bits(V))                 # the source is read only
    for c in list(dst.values()) + [whole, src]:
        c.close()


def test_exact_copy_between_families_with_different_padding():
    """An NMF context with num_bases <= 32 pads 448 columns to 512: both directions of a whole copy cross leading dimensions,
    and a gathered destination has a pad wider than 64 columns."""
    c = sc.NMF_PADDED
    V = sc.gather_data(c["rows"], c["n"])
    plain = holder(V)
    nmf = _lib.Context(_lib.ALGO_NMF, c["rows"], c["n"], c["num_bases"])
    nmf.set_v_gather(plain)
    assert np.array_equal(bits(nmf.get_v_dense()), bits(V))
    back = _lib.Context(_lib.ALGO_CUR, c["rows"], c["n"], 1)
    back.set_v_gather(nmf)
    assert np.array_equal(bits(back.get_v_dense()), bits(V))
    idx = sc.gather_index("random_repeats", c["n"], c["nsel"])
    small = _lib.Context(_lib.ALGO_NMF, c["rows"], c["nsel"], c["num_bases"])
    small.set_v_gather(nmf, idx)
    assert np.array_equal(bits(small.get_v_dense()), bits(V[:, idx]))
    # a destination that held other data, wider than the new columns' neighbours: refilled whole, pad included
    small.set_v_gather(plain, idx[::-1].copy())
    assert np.array_equal(bits(small.get_v_dense()), bits(V[:, idx[::-1]]))


# ---- indistinguishable from an upload ----------------------------------------------------------------------------------------
def _pair(cls, V, idx, counter, **kw):
    """(model whose device V was gathered from a holder of V, model that uploads the same columns)."""
    src = pymf_amd.NMF(V, num_bases=1)
    src.upload_data()
    before = counter["calls"]
    a = cls(V[:, idx], **kw)
    a.adopt_data_from(src, idx)
    assert counter["calls"] == before                                       # no host upload behind the gather
    b = cls(np.ascontiguousarray(V[:, idx]), **kw)
    return a, b


@pytest.fixture
def uploads(monkeypatch):
    counter = {"calls": 0, "bytes": 0}
    real = _lib.Context.set_v_dense

    def counting(self, V):
        counter["calls"] += 1
        counter["bytes"] += int(np.asarray(V).shape[0]) * int(np.asarray(V).shape[1]) * 4
        return real(self, V)
    monkeypatch.setattr(_lib.Context, "set_v_dense", counting)
    return counter


@pytest.mark.parametrize("name", ["NMF", "NMFALS"])
def test_gathered_context_runs_like_an_uploaded_one(name, uploads):
    V = sc.sub_data(29, 300)
    idx = sc.gather_index("random_repeats", 300, 17)
    cls = getattr(pymf_amd, name)
    a, b = _pair(cls, V, idx, uploads, num_bases=4)
    rng = np.random.RandomState(2)
    W0, H0 = rng.random_sample((29, 4)), rng.random_sample((4, 17))
    for mdl in (a, b):
        mdl.W, mdl.H = W0.copy(), H0.copy()
        mdl.factorize(niter=2)
    assert uploads["calls"] == 2                                            # the holder's and b's: a never uploaded
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.ferr, b.ferr)
    assert a.ferr.shape == (2,) and np.all(np.isfinite(a.ferr))


def test_gathered_kmeans_runs_like_an_uploaded_one(uploads):
    V = sc.sub_data(29, 300)
    idx = sc.gather_index("random_repeats", 300, 17)
    a, b = _pair(pymf_amd.Kmeans, V, idx, uploads, num_bases=4)
    for mdl in (a, b):
        random.seed(9)
        mdl.factorize(niter=2)
    assert uploads["calls"] == 2
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.ferr, b.ferr)
    assert np.array_equal(a.assigned, b.assigned)


def test_gathered_sivm_selects_like_an_uploaded_one(uploads):
    V = sc.sub_data(29, 300)
    idx = sc.gather_index("ascending", 300, 17)                             # no repeats: duplicate columns leave H not unique
    a, b = _pair(pymf_amd.SIVM, V, idx, uploads, num_bases=4)
    for mdl in (a, b):
        mdl.factorize()
    assert uploads["calls"] == 2
    assert a.select == b.select and len(set(a.select)) == 4
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.ferr, b.ferr)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_as_it_was():
    rows, n, nsel = 29, 300, 17
    V = sc.gather_data(rows, n)
    src = holder(V)
    old = sc.gather_data(rows, nsel, seed=77)
    dst = holder(old)
    good = sc.gather_index("ascending", n, nsel)

    def refused(call, pattern):
        with pytest.raises(_lib.PmfError) as e:
            call()
        assert e.value.code == _lib.PMF_EINVAL, str(e.value)
        assert pattern in str(e.value), str(e.value)
        assert np.array_equal(bits(dst.get_v_dense()), bits(old)), pattern

    bad = good.copy(); bad[5] = -1
    refused(lambda: dst.set_v_gather(src, bad), "index out of range: idx[5] = -1")
    bad = good.copy(); bad[16] = n
    refused(lambda: dst.set_v_gather(src, bad), "index out of range: idx[16] = 300")
    refused(lambda: dst.set_v_gather(src, good[:16]), "nsel != dst->n")
    refused(lambda: dst.set_v_gather(src), "nsel != dst->n")              # the whole copy into a narrower context
    other_rows = holder(sc.gather_data(rows + 1, n))
    refused(lambda: dst.set_v_gather(other_rows, good), "src->m != dst->m")
    empty = _lib.Context(_lib.ALGO_CUR, rows, n, 1)
    refused(lambda: dst.set_v_gather(empty, good), "src has no data")
    refused(lambda: dst.set_v_gather(dst, np.arange(nsel)), "src and dst are the same context")
    # CSR and CSC sources
    D = np.where(np.random.RandomState(3).random_sample((rows, n)) < 0.2, np.float32(1.5), np.float32(0.0))
    r_, c_ = np.nonzero(D)                                     # (row-major order: ascending columns within a row)
    csr = _lib.Context(_lib.ALGO_CUR, rows, n, 1)
    csr.set_v_csr(np.concatenate(([0], np.cumsum(np.bincount(r_, minlength=rows)))), c_, D[r_, c_])
    refused(lambda: dst.set_v_gather(csr, good), "src holds CSR data")
    c2, r2 = np.nonzero(D.T)                                   # (ascending rows within a column)
    csc = _lib.Context(_lib.ALGO_SIVM, rows, n, 4)
    csc.set_v_csc(np.concatenate(([0], np.cumsum(np.bincount(c2, minlength=n)))), r2, D[r2, c2])
    refused(lambda: dst.set_v_gather(csc, good), "src holds CSC data")
    # a source with a streamed pass open
    streamed = holder(np.abs(V) + 1.0, algo=_lib.ALGO_NMF, k=4)
    streamed.set_w(np.ones((rows, 4))); streamed.set_h(np.ones((4, n)))
    streamed.stream_begin(resid=True)
    refused(lambda: dst.set_v_gather(streamed, good), "src is in streamed mode")
    # a multi-rank world on either side (a host transport installed makes a context multi-rank)
    ranked = holder(V)
    ranked.set_host_allreduce(lambda a: a)
    refused(lambda: dst.set_v_gather(ranked, good), "src belongs to a multi-rank world")
    ranked_dst = holder(old)
    ranked_dst.set_host_allreduce(lambda a: a)
    with pytest.raises(_lib.PmfError) as e:
        ranked_dst.set_v_gather(src, good)
    assert e.value.code == _lib.PMF_EINVAL and "dst belongs to a multi-rank world" in str(e.value)
    assert np.array_equal(bits(ranked_dst.get_v_dense()), bits(old))
    if _lib.device_count() >= 2:
        far = _lib.Context(_lib.ALGO_CUR, rows, n, 1, device=1)
        far.set_v_dense(V)
        refused(lambda: dst.set_v_gather(far, good), "different devices")
    # the download's own refusal
    with pytest.raises(_lib.PmfError) as e:
        empty.get_v_dense()
    assert e.value.code == _lib.PMF_EINVAL and "has no data" in str(e.value)
    # ... and after all that the destination still takes a gather
    dst.set_v_gather(src, good)
    assert np.array_equal(bits(dst.get_v_dense()), bits(V[:, good]))


# ---- event ordering -----------------------------------------------------------------------------------------------------------
def test_event_ordering_gives_what_explicit_synchronisation_gives():
    rows, n, nsel, k = 300, 5000, 1030, 16
    V1, V2 = sc.sub_data(rows, n, seed=21), sc.sub_data(rows, n, seed=22)
    idx = sc.gather_index("random_repeats", n, nsel)
    rng = np.random.RandomState(4)
    W0, H0 = rng.random_sample((rows, k)), rng.random_sample((k, n))
    Wd, Hd = rng.random_sample((rows, k)), rng.random_sample((k, nsel))

    def run(sync):
        src = holder(V1, algo=_lib.ALGO_NMF, k=k)
        dst = _lib.Context(_lib.ALGO_NMF, rows, nsel, k)
        src.set_w(W0); src.set_h(H0)
        dst.set_w(Wd); dst.set_h(Hd)
        wait = (lambda: (src.synchronize(), dst.synchronize())) if sync else (lambda: None)
        src.update_w(); src.update_h()                         # an iteration just enqueued on the source's stream
        wait()
        dst.set_v_gather(src, idx)                             # reads the source's V behind that iteration
        wait()
        src.update_w(); src.update_h()                         # another iteration on the source, while the gather may still run
        wait()
        src.set_v_dense(V2)                                    # the source's V is written again: only after the gather has read it
        wait()
        dst.update_w(); dst.update_h()
        out = (dst.get_v_dense(), dst.get_w(), dst.get_h(), dst.frobenius(), src.get_w(), src.get_h(), src.get_v_dense())
        src.close(); dst.close()
        return out

    free, synced = run(False), run(True)
    assert np.array_equal(bits(free[0]), bits(V1[:, idx]))
    assert np.array_equal(bits(free[6]), bits(V2))
    for a, b in zip(free, synced):
        assert np.array_equal(np.asarray(a), np.asarray(b))
