"""Host-side logic of the drop-in classes that needs no GPU: which factorize() path is taken (template
method, nmf.py:182-202), the W / H attribute semantics, the digest-based change detection and the
streamed-mode switches."""
import numpy as np
import pytest

import pymf_amd
from pymf_amd import _lib
from pymf_amd.rnmf import RNMF


def test_shipped_classes_take_the_one_call_path():
    V = np.ones((6, 5), dtype=np.float32)
    for cls in (pymf_amd.NMF, pymf_amd.SNMF, pymf_amd.NMFALS, pymf_amd.NMFNNLS, pymf_amd.BNMF, RNMF):
        assert not cls(V, num_bases=2)._hooks_overridden(), cls.__name__


def test_overridden_hooks_are_detected():
    V = np.ones((6, 5), dtype=np.float32)

    class A(pymf_amd.NMF):
        def update_h(self):
            pymf_amd.NMF.update_h(self)

    class B(pymf_amd.SNMF):
        def converged(self, i):
            return False

    class C(pymf_amd.BNMF):          # a subclass that overrides nothing: still the fast path
        extra = 1

    class D(A):                      # inherits A's override
        pass

    assert A(V)._hooks_overridden() and B(V)._hooks_overridden() and D(V)._hooks_overridden()
    assert not C(V)._hooks_overridden()
    m = pymf_amd.NMF(V)
    m.frobenius_norm = lambda: 0.0   # instance-level replacement
    assert m._hooks_overridden()


def test_w_h_attribute_semantics():
    """W and H behave like the reference's plain attributes: absent until created (nmf.py:173-177 tests
    hasattr), assignable, deletable; assigning marks the device copy stale."""
    m = pymf_amd.NMF(np.ones((6, 5), dtype=np.float32), num_bases=2)
    assert not hasattr(m, "W") and not hasattr(m, "H")
    with pytest.raises(AttributeError):
        m.W
    W = np.random.rand(6, 2)
    m.W = W
    assert m.W is W and hasattr(m, "W") and m._w_fp is None
    m._w_fp = ("something",)
    m.W = W.copy()
    assert m._w_fp is None
    del m.W
    assert not hasattr(m, "W")
    with pytest.raises(AttributeError):
        del m.W
    assert m.frobenius_norm() == -123456          # nmf.py:112: no W/H yet -> the sentinel, no device needed


def test_fingerprint_follows_in_place_edits():
    from pymf_amd.nmf import _fingerprint
    W = np.random.RandomState(0).rand(1000, 8)
    f0 = _fingerprint(W)
    assert _fingerprint(W) == f0
    W[[1, 2]] = W[[2, 1]]
    assert _fingerprint(W) != f0


def test_stream_switches():
    V = np.ones((200, 5), dtype=np.float32)
    for cls, ok in ((pymf_amd.NMF, True), (pymf_amd.BNMF, True), (pymf_amd.SNMF, True), (pymf_amd.NMFALS, True), (RNMF, False)):
        m = cls(V, num_bases=2)
        assert m._stream_rows() == 0
        m.stream_rows = 100
        assert m._stream_rows() == (128 if ok else 0), cls.__name__       # rounded up to 64 rows


def test_row_span_single_rank():
    m = pymf_amd.NMF(np.ones((37, 5), dtype=np.float32), num_bases=2)
    assert m._row_span() == (0, 37, 37) and m._global_rows() == 37


class _CountingCtx(object):
    """Test double of _lib.Context (NumPy float64 math through the oracle's functions) that counts what
    crosses the boundary: uploads of W / H and downloads of them."""

    def __init__(self, m, n, k):
        self.m, self.n, self.k = m, n, k
        self.up = {"W": 0, "H": 0, "V": 0}
        self.down = {"W": 0, "H": 0}

    def set_v_dense(self, V):
        self.V = np.asarray(V, dtype=np.float64)
        self.up["V"] += 1

    def set_w(self, W):
        self.W = np.array(W, dtype=np.float64)
        self.up["W"] += 1

    def set_h(self, H):
        self.H = np.array(H, dtype=np.float64)
        self.up["H"] += 1

    def get_w(self):
        self.down["W"] += 1
        return self.W.astype(np.float32)

    def get_h(self):
        self.down["H"] += 1
        return self.H.astype(np.float32)

    def invalidate_v(self):
        pass

    def factorize(self, niter, compute_w=True, compute_h=True, compute_err=True, conv_eps=1e-8):
        import oracle
        for _ in range(niter):
            if compute_w:
                oracle.nmf_update_w(self.V, self.W, self.H)
            if compute_h:
                oracle.nmf_update_h(self.V, self.W, self.H)
        return (np.ones(max(niter, 1)) if compute_err else None), niter, -1


def _model_with_double(m=40, n=12, k=3, seed=0):
    rs = np.random.RandomState(seed)
    mdl = pymf_amd.NMF(rs.rand(m, n).astype(np.float32), num_bases=k)
    mdl._ctx = _CountingCtx(m, n, k)
    mdl.W, mdl.H = rs.rand(m, k), rs.rand(k, n)
    return mdl


def test_factors_stay_on_the_device_between_calls_when_nobody_can_see_the_host_arrays():
    """`mdl.factorize(); mdl.factorize(); mdl.W`: the host arrays belong to the object alone, so they are
    brought up to date when they are read -- one download of W and H in all, one upload."""
    import oracle
    mdl = _model_with_double()
    ref = oracle.NMFOracle(mdl.data, num_bases=3)
    ref.W, ref.H = mdl.__dict__["_W"].copy(), mdl.__dict__["_H"].copy()
    ctx = mdl._ctx
    mdl.factorize(niter=2, compute_err=False)
    mdl.factorize(niter=3, compute_err=False)
    assert ctx.up == {"W": 1, "H": 1, "V": 1} and ctx.down == {"W": 0, "H": 0}
    ref.factorize(niter=5, compute_err=False)
    np.testing.assert_allclose(mdl.W, ref.W, rtol=1e-6)      # the read refreshes (float32 transport)
    np.testing.assert_allclose(mdl.H, ref.H, rtol=1e-6)
    assert ctx.down == {"W": 1, "H": 1}
    mdl.factorize(niter=1, compute_err=False)                 # handed out, unchanged: digested, not uploaded
    assert ctx.up["W"] == 1 and ctx.up["H"] == 1


def test_held_arrays_are_updated_in_place_after_every_call():
    """`w = mdl.W; mdl.factorize(); w` has changed (nmf.py:131-132 writes in place): an array somebody
    else holds -- a name, or a view of it -- is refreshed eagerly."""
    mdl = _model_with_double(seed=1)
    w = mdl.W
    before = w.copy()
    mdl.factorize(niter=1, compute_err=False)
    assert mdl._ctx.down["W"] == 1 and not np.array_equal(w, before) and mdl.W is w
    assert mdl._ctx.down["H"] == 0                            # nobody holds H
    hv = mdl.H[:1]                                            # a live VIEW keeps the base reachable
    assert mdl._ctx.down["H"] == 1
    mdl.factorize(niter=1, compute_err=False)
    assert mdl._ctx.down["H"] == 2
    del hv


def test_in_place_edit_through_the_attribute_reaches_the_device():
    mdl = _model_with_double(seed=2)
    mdl.factorize(niter=1, compute_err=False)
    mdl.H[0, 0] += 1.0                                        # read (refresh) + edit in place
    expect = mdl.__dict__["_H"].copy()
    mdl.factorize(niter=0, compute_err=False)
    assert mdl._ctx.up["H"] == 2
    np.testing.assert_allclose(mdl._ctx.H, expect.astype(np.float32), rtol=1e-6)


def test_eager_factors_switch_and_views_of_user_memory():
    mdl = _model_with_double(seed=3)
    mdl.eager_factors = True
    mdl.factorize(niter=1, compute_err=False)
    assert mdl._ctx.down == {"W": 1, "H": 1}
    big = np.random.rand(40, 8)
    m2 = _model_with_double(seed=4)
    m2.W = big[:, :3]                                         # a view of the caller's buffer: never lazy
    assert m2._held_elsewhere("W")
    m2.factorize(niter=1, compute_err=False)
    assert m2._ctx.down["W"] == 1
    np.testing.assert_allclose(big[:, :3], m2._ctx.W, rtol=1e-6)


def test_pickling_flushes_the_host_arrays():
    import pickle
    mdl = _model_with_double(seed=5)
    mdl.factorize(niter=2, compute_err=False)
    assert mdl._host_stale == {"W", "H"}
    clone = pickle.loads(pickle.dumps(mdl))
    assert clone._ctx is None and clone._host_stale == set()
    np.testing.assert_allclose(clone.__dict__["_W"], mdl._ctx.W, rtol=1e-6)


def test_failed_w_step_leaves_the_previous_factors_like_the_reference():
    """snmf.py:69-70: np.linalg.inv raises BEFORE W is rebound, so after a LinAlgError at iteration i the object
    holds iteration i-1's W and H.  Here the failing call leaves garbage in the device W: before every W step
    that may fail the device W is snapshot (device to device) and put back when the step raised; the factors,
    still device-resident, reach the host when they are read."""
    import oracle

    class Ctx(_CountingCtx):
        calls = 0

        def snapshot_w(self):                           # pmf_snapshot_w: a device-to-device copy
            self.Wsnap = self.W.copy()

        def restore_w(self):
            self.W = self.Wsnap.copy()

        def update_w(self):
            Ctx.calls += 1
            if Ctx.calls == 3:
                self.W[:] = np.nan                      # what a singular H H^T leaves behind on the device
                raise _lib.PmfError("SNMF: H H^T is singular")
            oracle.nmf_update_w(self.V, self.W, self.H)

        def update_h(self):
            oracle.nmf_update_h(self.V, self.W, self.H)

    rs = np.random.RandomState(7)
    V = rs.rand(30, 10).astype(np.float32)
    mdl = pymf_amd.SNMF(V, num_bases=3)
    mdl._ctx = Ctx(30, 10, 3)
    W0, H0 = rs.rand(30, 3), rs.rand(3, 10)
    mdl.W, mdl.H = W0.copy(), H0.copy()
    with pytest.raises(_lib.PmfError):
        mdl.factorize(niter=5, show_progress=True, compute_err=False)     # hook loop; the third W step fails
    Wr, Hr = W0.copy(), H0.copy()
    for _ in range(2):
        oracle.nmf_update_w(V.astype(np.float64), Wr, Hr)
        oracle.nmf_update_h(V.astype(np.float64), Wr, Hr)
    np.testing.assert_allclose(mdl.W, Wr, rtol=1e-6)
    np.testing.assert_allclose(mdl.H, Hr, rtol=1e-6)
    assert np.isfinite(mdl.W).all()


def test_success_then_failing_one_call_factorize_keeps_a_consistent_pair():
    """Advisor (round 3): after a successful lazy factorize() W and H live on the device alone; a factorize() that
    raises afterwards must not declare the untouched (older) host arrays current.  SNMF (a class whose W step may
    fail): the pair before the failing call survives -- W through the device snapshot, H through the flush that
    precedes such a call.  NMF: factors that lived on the device alone keep doing so."""
    import oracle

    class Ctx(_CountingCtx):
        fail_next = False

        def snapshot_w(self):
            self.Wsnap = self.W.copy()

        def restore_w(self):
            self.W = self.Wsnap.copy()

        def factorize(self, niter, *a, **kw):
            if self.fail_next:
                self.W[:] = np.nan                      # what a singular H H^T leaves behind on the device
                self.H[:] = np.nan
                raise np.linalg.LinAlgError("Singular matrix")
            return _CountingCtx.factorize(self, niter, *a, **kw)

    rs = np.random.RandomState(11)
    V = rs.rand(30, 10).astype(np.float32)
    for cls in (pymf_amd.SNMF, pymf_amd.NMF):
        mdl = cls(V, num_bases=3)
        mdl._ctx = Ctx(30, 10, 3)
        W0, H0 = rs.rand(30, 3), rs.rand(3, 10)
        mdl.W, mdl.H = W0.copy(), H0.copy()
        mdl.factorize(niter=2, compute_err=False)                     # success: both factors device-only now
        assert mdl._host_stale == {"W", "H"}
        Wr, Hr = W0.copy(), H0.copy()
        for _ in range(2):
            oracle.nmf_update_w(V.astype(np.float64), Wr, Hr)
            oracle.nmf_update_h(V.astype(np.float64), Wr, Hr)
        mdl._ctx.fail_next = True
        with pytest.raises(np.linalg.LinAlgError):
            mdl.factorize(niter=3, compute_err=False)
        if cls is pymf_amd.SNMF:
            np.testing.assert_allclose(mdl.W, Wr, rtol=1e-6)          # call 1's result, not W0
            np.testing.assert_allclose(mdl.H, Hr, rtol=1e-6)          # ... and not H0
            # and the next call computes from that pair
            mdl._ctx.fail_next = False
            mdl.factorize(niter=0, compute_err=False)
            np.testing.assert_allclose(mdl._ctx.H, Hr.astype(np.float32), rtol=1e-6)
        else:
            # nothing better than the device copies exists: they stay the current ones (never W0 / H0 again)
            assert mdl._host_stale == {"W", "H"}
            assert not np.array_equal(mdl.__dict__["_W"], Wr)         # host array untouched, and not declared current
            assert mdl._w_fp is not None or "W" in mdl._host_stale


def test_copies_share_no_bookkeeping_with_the_original():
    import copy
    mdl = _model_with_double(seed=6)
    mdl.factorize(niter=1, compute_err=False)
    clone = copy.copy(mdl)
    assert clone._host_stale is not mdl._host_stale and clone._handed is not mdl._handed
    mdl.factorize(niter=1, compute_err=False)                         # stale again on the original only
    assert clone._host_stale == set() and clone._ctx is None


def test_float64_data_warns_once_per_object():
    import warnings
    mdl = _model_with_double(seed=8)
    mdl.data = mdl.data.astype(np.float64)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        mdl.factorize(niter=1, compute_err=False)
        mdl.check_data = True
        mdl.factorize(niter=1, compute_err=False)
    hits = [r for r in rec if issubclass(r.category, pymf_amd.nmf.PrecisionWarning)]
    assert len(hits) == 1 and "float32" in str(hits[0].message)


class _LateCtx(_CountingCtx):
    """The counting double with the four calls the late data check needs; a log of the boundary traffic in order."""

    def __init__(self, m, n, k):
        _CountingCtx.__init__(self, m, n, k)
        self.log, self.aborted = [], False

    def snapshot_w(self):
        self.log.append("snapshot_w"); self._ws = self.W.copy()

    def snapshot_h(self):
        self.log.append("snapshot_h"); self._hs = self.H.copy()

    def restore_w(self):
        self.log.append("restore_w"); self.W = self._ws.copy()

    def restore_h(self):
        self.log.append("restore_h"); self.H = self._hs.copy()

    def abort(self, on=True):
        self.log.append("abort(%d)" % (1 if on else 0)); self.aborted = bool(on)

    def set_v_dense(self, V):
        self.log.append("set_v"); _CountingCtx.set_v_dense(self, V)

    def factorize(self, niter, *a, **kw):
        import time
        self.log.append("factorize(%d)" % niter)
        time.sleep(0.05)                                      # (the digest thread finishes first: its abort is on record)
        return _CountingCtx.factorize(self, niter, *a, **kw)


def test_late_data_check_restarts_the_loop_when_the_bytes_changed():
    """Round 5: the digest of `data` runs on a second thread beside the device loop.  Unchanged bytes: snapshots, one loop,
    nothing else.  Bytes edited in place since the upload: the loop is asked to stop, W and H are put back from the device-side
    copies, the new bytes go up, the loop runs again -- and the result is what a check-first object computes."""
    import oracle
    rs = np.random.RandomState(8)
    V = rs.rand(64, 16).astype(np.float32)
    W0, H0 = rs.rand(64, 3), rs.rand(3, 16)

    def model(late):
        mdl = pymf_amd.NMF(V.copy(), num_bases=3)
        mdl._ctx = _LateCtx(64, 16, 3)
        mdl._LATE_DATA_CHECK, mdl._LATE_DATA_CHECK_MIN_BYTES = late, 0
        mdl.W, mdl.H = W0.copy(), H0.copy()
        return mdl
    a, b = model(True), model(False)
    for mdl in (a, b):
        mdl.factorize(niter=2, compute_err=False)             # the first call uploads: checked in front, in both
    assert "snapshot_w" not in a._ctx.log
    a._ctx.log[:] = []
    a.factorize(niter=2, compute_err=False); b.factorize(niter=2, compute_err=False)
    # (the trailing abort(0): however the call ends, the context's abort request is withdrawn -- round-5 advisor: a flag left
    #  set by an interrupted call made the NEXT loop return at once)
    assert a._ctx.log == ["snapshot_w", "snapshot_h", "factorize(2)", "abort(0)"], a._ctx.log
    a._ctx.log[:] = []
    for mdl in (a, b):
        mdl.data[5, 3] += 0.5                                 # in place: same object, new bytes
    a.factorize(niter=3, compute_err=False); b.factorize(niter=3, compute_err=False)
    assert a._ctx.log == ["snapshot_w", "snapshot_h", "factorize(3)", "abort(1)", "abort(0)", "restore_w", "restore_h", "set_v", "factorize(3)", "abort(0)"] or \
        a._ctx.log == ["snapshot_w", "snapshot_h", "abort(1)", "factorize(3)", "abort(0)", "restore_w", "restore_h", "set_v", "factorize(3)", "abort(0)"], a._ctx.log
    assert not a._ctx.aborted and a._ctx.up["V"] == 2 == b._ctx.up["V"]
    np.testing.assert_array_equal(a._ctx.W, b._ctx.W)
    np.testing.assert_array_equal(a._ctx.H, b._ctx.H)
    np.testing.assert_array_equal(a.W, b.W)


def test_an_interrupted_call_does_not_leave_the_abort_request_behind():
    """Round-5 advisor: pmf_abort is sticky.  The digest thread sets it when `data` changed under the running loop; if the main
    thread then leaves factorize() without reaching the restart (a KeyboardInterrupt behind the loop), the flag stayed set and
    the NEXT pmf_factorize returned at once with iters_done = 0 and no error.  Now the call ends -- however it ends -- with the
    digest thread joined and the request withdrawn."""
    rs = np.random.RandomState(9)
    V = rs.rand(64, 16).astype(np.float32)

    class Interrupted(_LateCtx):
        boom = False

        def factorize(self, niter, *a, **kw):
            out = _LateCtx.factorize(self, niter, *a, **kw)
            if self.boom:
                raise KeyboardInterrupt()
            return out
    mdl = pymf_amd.NMF(V, num_bases=3)
    mdl._ctx = Interrupted(64, 16, 3)
    mdl._LATE_DATA_CHECK, mdl._LATE_DATA_CHECK_MIN_BYTES = True, 0
    mdl.W, mdl.H = rs.rand(64, 3), rs.rand(3, 16)
    mdl.factorize(niter=2, compute_err=False)                 # the first call uploads
    V[3, 3] += 1.0                                            # edited in place: the digest thread will ask the loop to stop ...
    mdl._ctx.boom = True
    mdl._ctx.log[:] = []
    with pytest.raises(KeyboardInterrupt):                    # ... and the main thread never gets to the restart
        mdl.factorize(niter=3, compute_err=False)
    assert "abort(1)" in mdl._ctx.log and mdl._ctx.log[-1] == "abort(0)", mdl._ctx.log
    assert mdl._ctx.aborted is False


class _CnmfCtx(_CountingCtx):
    """The counting double with the calls pymf_amd.CNMF makes (set_g / get_g / get_h64 / cnmf_init / last_loop_ms), a log of
    the boundary traffic in order, and arithmetic that is only recognisable: an iteration adds 1 to G (W = V G) and to H."""

    def __init__(self, m, n, k):
        _CountingCtx.__init__(self, m, n, k)
        self.up["G"] = self.down["G"] = 0
        self.log = []
        self.W = self.H = self.G = None

    def set_v_dense(self, V):
        self.log.append("set_v"); _CountingCtx.set_v_dense(self, V)

    def set_w(self, W):
        self.log.append("set_w"); _CountingCtx.set_w(self, W)

    def set_h(self, H):
        self.log.append("set_h"); _CountingCtx.set_h(self, H)

    def set_g(self, G):
        self.log.append("set_g"); self.G = np.array(G, dtype=np.float64); self.up["G"] += 1

    def get_g(self):
        self.down["G"] += 1
        return self.G.copy()

    def get_h64(self):
        self.down["H"] += 1
        return self.H.copy()

    def cnmf_init(self, sel, km_niter=10):
        self.log.append("cnmf_init")
        self.H = np.full((self.k, self.n), 0.2)
        if self.G is None:
            self.G = np.full((self.n, self.k), 0.01)
        if self.W is None:
            self.W = self.V @ self.G

    def factorize(self, niter, compute_w=True, compute_h=True, compute_err=True, conv_eps=1e-8):
        self.log.append("factorize(%d)" % niter)
        for _ in range(niter):
            if compute_w:
                self.G = self.G + 1.0
                self.W = self.V @ self.G
            if compute_h:
                self.H = self.H + 1.0
        return np.arange(max(niter, 1), 0, -1.0), niter, -1

    def last_loop_ms(self):
        return 0.25


def _cnmf_with_double(m=20, n=10, k=3, seed=0, cls=None):
    rs = np.random.RandomState(seed)
    mdl = (cls or pymf_amd.CNMF)(rs.randn(m, n).astype(np.float32), num_bases=k)
    mdl._ctx = _CnmfCtx(m, n, k)
    return mdl


def test_cnmf_factors_stay_on_the_device_until_they_are_read():
    """init through factorize(), a second factorize(), reads of .G / .H / .W: nothing goes up but `data`, every factor comes
    down once, when it is read; G comes back in place (cnmf.py:174), H and W as new float64 arrays (cnmf.py:167,175)."""
    mdl = _cnmf_with_double()
    ctx = mdl._ctx
    mdl.factorize(niter=2)
    assert ctx.log == ["set_v", "cnmf_init", "factorize(2)"], ctx.log
    assert mdl._host_stale == {"G", "H", "W"} and mdl._handed == set()
    assert mdl._g_fp is None and mdl._h_fp is None and mdl._w_fp is None
    assert ctx.up == {"W": 0, "H": 0, "G": 0, "V": 1} and ctx.down == {"W": 0, "H": 0, "G": 0}
    assert mdl.last_call_ms["loop"] == 0.25 and set(mdl.last_call_ms) >= {"init", "upload", "loop", "total"}
    np.testing.assert_array_equal(mdl.ferr, [2.0, 1.0])
    mdl.factorize(niter=3)
    assert ctx.log[3:] == ["factorize(3)"] and mdl._host_stale == {"G", "H", "W"}
    assert ctx.up == {"W": 0, "H": 0, "G": 0, "V": 1} and ctx.down == {"W": 0, "H": 0, "G": 0}
    g_host = mdl.__dict__["_G"]
    np.testing.assert_array_equal(mdl.G, np.full((10, 3), 5.01))
    assert mdl.__dict__["_G"] is g_host                               # in place
    del g_host
    assert ctx.down == {"W": 0, "H": 0, "G": 1} and mdl._host_stale == {"H", "W"} and mdl._handed == {"G"}
    assert mdl._g_fp is not None
    h_host = mdl.__dict__["_H"]
    np.testing.assert_array_equal(mdl.H, np.full((3, 10), 5.2))
    assert mdl.__dict__["_H"] is not h_host and mdl.H.dtype == np.float64     # rebound
    assert ctx.down == {"W": 0, "H": 1, "G": 1} and mdl._host_stale == {"W"}
    w_host = mdl.__dict__["_W"]
    np.testing.assert_array_equal(mdl.W, ctx.W.astype(np.float32).astype(np.float64))
    assert mdl.__dict__["_W"] is not w_host and mdl.W.dtype == np.float64     # rebound
    assert ctx.down == {"W": 1, "H": 1, "G": 1} and mdl._host_stale == set() and mdl._handed == {"G", "H", "W"}
    mdl.factorize(niter=1)                                            # handed out, unchanged: digested, not uploaded
    assert ctx.up == {"W": 0, "H": 0, "G": 0, "V": 1} and mdl._handed == set()
    assert mdl._host_stale == {"G", "H", "W"} and ctx.down == {"W": 1, "H": 1, "G": 1}


def test_cnmf_in_place_edit_of_g_reaches_the_device_and_setters_run_g_h_w():
    mdl = _cnmf_with_double(seed=1)
    ctx = mdl._ctx
    mdl.factorize(niter=1)
    mdl.G[0, 0] += 0.5                                                # read (refresh, in place) + edit
    assert ctx.down["G"] == 1 and mdl._host_stale == {"H", "W"}
    expect = mdl.__dict__["_G"].copy()
    ctx.log[:] = []
    mdl.factorize(niter=0)
    assert ctx.log == ["set_g", "factorize(0)"], ctx.log               # H and W: the device copies are the newer ones
    np.testing.assert_array_equal(ctx.G, expect)
    assert mdl._host_stale == {"H", "W"}                              # no iteration ran: G's host array stays current
    # all three assigned: G, H, W in that order (the library's w_replaced / h_replaced bookkeeping sees them so)
    rs = np.random.RandomState(3)
    mdl.W, mdl.H, mdl.G = rs.rand(20, 3), rs.rand(3, 10), rs.rand(10, 3)
    assert mdl._host_stale == set() and mdl._g_fp is None and mdl._h_fp is None and mdl._w_fp is None
    ctx.log[:] = []
    mdl.factorize(niter=1, compute_w=False)
    assert ctx.log == ["set_g", "set_h", "set_w", "factorize(1)"], ctx.log
    assert mdl._host_stale == {"H"}                                   # compute_w=False: G and W did not move
    ctx.log[:] = []
    mdl.factorize(niter=1, compute_h=False)
    assert ctx.log == ["factorize(1)"] and mdl._host_stale == {"G", "H", "W"}     # a W step moves W and G
    mdl.G = np.arange(30).reshape(10, 3)
    with pytest.raises(TypeError):
        mdl.factorize(niter=1)                                        # an integer G, as an integer W in NMF


def test_cnmf_factors_that_do_not_exist_yet_are_skipped_by_the_upload():
    """init_h synchronises before H exists: a G the caller set goes up, what is missing is left to pmf_cnmf_init;
    H and G given but no W: W = data G on the device."""
    mdl = _cnmf_with_double(seed=2)
    G0 = np.random.RandomState(4).rand(10, 3)
    mdl.G = G0
    mdl.factorize(niter=1)
    assert mdl._ctx.log == ["set_v", "set_g", "cnmf_init", "factorize(1)"], mdl._ctx.log
    # G0 is held by the caller: brought up to date in place, at once
    assert mdl._host_stale == {"H", "W"} and mdl.__dict__["_G"] is G0 and mdl._ctx.down["G"] == 1
    np.testing.assert_array_equal(G0, mdl._ctx.G)
    m2 = _cnmf_with_double(seed=2)
    m2.H, m2.G = np.ones((3, 10)), G0.copy()
    m2.factorize(niter=0)
    assert m2._ctx.log == ["set_v", "set_g", "set_h", "factorize(0)"], m2._ctx.log
    assert m2._host_stale == {"W"} and m2._w_fp is None


def test_cnmf_held_arrays_are_refreshed_after_every_call():
    mdl = _cnmf_with_double(seed=5)
    mdl.factorize(niter=1)
    g, h = mdl.G, mdl.H
    down = dict(mdl._ctx.down)
    mdl.factorize(niter=2)
    assert mdl.G is g and g[0, 0] == 3.01                             # in place
    assert mdl.H is not h and h[0, 0] == 1.2 and mdl.H[0, 0] == 3.2   # rebound: the caller's old array is left alone
    assert mdl._ctx.down == {"W": down["W"], "H": down["H"] + 1, "G": down["G"] + 1}
    assert mdl._host_stale == {"W"}
    mdl.eager_factors = True
    mdl.factorize(niter=1, compute_h=False)
    assert mdl._host_stale == set() and mdl._ctx.down == {"W": down["W"] + 1, "H": down["H"] + 1, "G": down["G"] + 2}


def test_cnmf_pickle_and_copy_flush_all_three_factors():
    import copy
    import pickle
    mdl = _cnmf_with_double(seed=6)
    mdl.factorize(niter=2)
    assert mdl._host_stale == {"G", "H", "W"}
    clone = pickle.loads(pickle.dumps(mdl))
    assert mdl._ctx.down == {"W": 1, "H": 1, "G": 1} and mdl._host_stale == set()
    assert clone._ctx is None and clone._host_stale == set() and clone._handed == set()
    assert clone._g_fp is None and clone._h_fp is None and clone._w_fp is None and clone._v_src is None
    np.testing.assert_array_equal(clone.__dict__["_G"], mdl._ctx.G)
    np.testing.assert_array_equal(clone.__dict__["_H"], mdl._ctx.H)
    assert mdl._g_fp is not None and mdl._h_fp is not None and mdl._w_fp is not None
    mdl.factorize(niter=1)
    twin = copy.copy(mdl)
    assert mdl._ctx.down == {"W": 2, "H": 2, "G": 2}
    assert twin._host_stale is not mdl._host_stale and twin._handed is not mdl._handed
    mdl.factorize(niter=1)                                            # stale again on the original only
    assert twin._host_stale == set() and twin._ctx is None and twin._g_fp is None
    assert mdl._ctx.up == {"W": 0, "H": 0, "G": 0, "V": 1}


def test_cnmf_overridden_frobenius_norm_routes_through_the_hook_loop():
    """An overridden frobenius_norm is called every iteration (cnmf.py:156-187): one device iteration per loop turn,
    the factors staying on the device in between and afterwards."""
    seen = []

    class Mine(pymf_amd.CNMF):
        def frobenius_norm(self):
            seen.append(set(self._host_stale))
            return 100.0 / len(seen)

    mdl = _cnmf_with_double(seed=7, cls=Mine)
    assert mdl._hooks_overridden() and not _cnmf_with_double()._hooks_overridden()
    mdl.factorize(niter=3)
    assert mdl._ctx.log == ["set_v", "cnmf_init", "factorize(1)", "factorize(1)", "factorize(1)"], mdl._ctx.log
    assert seen == [{"G", "H", "W"}] * 3
    np.testing.assert_allclose(mdl.ferr, [100.0, 50.0, 100.0 / 3])
    assert mdl._host_stale == {"G", "H", "W"} and mdl._last_iters == 3
    assert mdl._ctx.down == {"W": 0, "H": 0, "G": 0} and mdl._ctx.up == {"W": 0, "H": 0, "G": 0, "V": 1}
    g = mdl.G
    mdl._ctx.log[:] = []
    mdl.factorize(niter=2, compute_h=False, compute_err=False)
    assert mdl._ctx.log == ["factorize(1)", "factorize(1)"] and len(seen) == 3
    assert mdl._ctx.down == {"W": 0, "H": 0, "G": 2}                  # the read, and one flush at the end of the loop
    assert g[0, 0] == 5.01 and mdl._host_stale == {"H", "W"}
    flat = _cnmf_with_double(seed=7)
    flat.frobenius_norm = lambda: 7.0                                 # instance-level, constant: converged() cuts at i == 2
    flat.factorize(niter=6)
    assert flat._ctx.log[2:] == ["factorize(1)"] * 3 and len(flat.ferr) == 2 and flat._last_iters == 3
