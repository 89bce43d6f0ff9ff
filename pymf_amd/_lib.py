"""ctypes binding of libpymf_hip.so (C ABI in include/pymf_hip.h).

The shared library is built in-tree by pymf_amd/csrc/build.py (hipcc,
--offload-arch=gfx950).  There is no CPU fallback: if the library is missing or
cannot be loaded, every entry point raises.
"""
import ctypes
import os

import numpy as np

# Single-node design (ranks of one xGMI node): keep RCCL's bootstrap off InfiniBand probing, which
# can stall communicator creation for minutes on hosts without a fabric; users may override both.
os.environ.setdefault("NCCL_IB_DISABLE", "1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PMF_LIB") or os.path.join(_HERE, "csrc", "libpymf_hip.so")   # PMF_LIB: A/B builds

PMF_OK, PMF_EINVAL, PMF_EHIP, PMF_ENCCL, PMF_ENOMEM, PMF_ESINGULAR, PMF_ENUMERIC = 0, -1, -2, -3, -4, -5, -6
ALGO_NMF, ALGO_NMFALS, ALGO_SNMF, ALGO_BNMF, ALGO_RNMF, ALGO_CNMF, ALGO_KMEANS, ALGO_CMEANS, ALGO_SIVM, ALGO_AA, ALGO_PCA = 0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12   # (7, 9: not assigned)
ALGO_CUR = 14   # (13: not assigned)
ALGO_GREEDY = 15
COMPUTE_W, COMPUTE_H, COMPUTE_ERR = 1, 2, 4
STREAM_RESID = 8
NCCL_ID_BYTES = 128
IPC_HANDLE_BYTES = 64

# every symbol include/pymf_hip.h declares: (name, restype, argtypes)
_c = ctypes
_ctx = _c.c_void_p
_fp = _c.POINTER(_c.c_float)
SYMBOLS = [
    ("pmf_device_count", _c.c_int, [_c.POINTER(_c.c_int32)]),
    ("pmf_nccl_unique_id", _c.c_int, [_c.c_void_p]),
    ("pmf_ctx_create", _c.c_int, [_c.POINTER(_ctx), _c.c_int32, _c.c_int64, _c.c_int64, _c.c_int32,
                                  _c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p]),
    ("pmf_ctx_destroy", _c.c_int, [_ctx]),
    ("pmf_last_error", _c.c_char_p, [_ctx]),
    ("pmf_set_v_dense_f32", _c.c_int, [_ctx, _c.c_void_p, _c.c_int64]),
    ("pmf_set_v_dense_f64", _c.c_int, [_ctx, _c.c_void_p, _c.c_int64]),
    ("pmf_set_v_csr_f32", _c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64]),
    ("pmf_check_csr", _c.c_int, [_c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int64]),
    ("pmf_set_v_csc_f32", _c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64]),
    ("pmf_check_csc", _c.c_int, [_c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_int64]),
    ("pmf_fill_v_uniform", _c.c_int, [_ctx, _c.c_uint64, _c.c_int64]),
    ("pmf_set_w_f32", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_get_w_f32", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_set_h_f32", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_get_h_f32", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_set_w_f64", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_get_w_f64", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_set_h_f64", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_get_h_f64", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_fill_w_uniform", _c.c_int, [_ctx, _c.c_uint64, _c.c_int64]),
    ("pmf_fill_h_uniform", _c.c_int, [_ctx, _c.c_uint64]),
    ("pmf_update_w", _c.c_int, [_ctx]),
    ("pmf_update_h", _c.c_int, [_ctx]),
    ("pmf_frobenius", _c.c_int, [_ctx, _c.POINTER(_c.c_double)]),
    ("pmf_factorize", _c.c_int, [_ctx, _c.c_int32, _c.c_uint32, _c.c_double, _c.c_void_p,
                                 _c.POINTER(_c.c_int32), _c.POINTER(_c.c_int32)]),
    ("pmf_set_lambda", _c.c_int, [_ctx, _c.c_double, _c.c_double]),
    ("pmf_get_lambda", _c.c_int, [_ctx, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("pmf_rnmf_update_s", _c.c_int, [_ctx]),
    ("pmf_rnmf_get_s_f32", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_rnmf_set_s_f32", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_nndsvd_init", _c.c_int, [_ctx, _c.POINTER(_c.c_int32)]),
    ("pmf_cnmf_init", _c.c_int, [_ctx, _c.c_void_p, _c.c_int32, _c.c_void_p]),
    ("pmf_set_g_f64", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_get_g_f64", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_cluster_get_assigned", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_cluster_set_assigned", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_sivm_get_select", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_sivm_get_volumes", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_gsat_start", _c.c_int, [_ctx, _c.c_void_p, _c.c_int32, _c.POINTER(_c.c_int32)]),
    ("pmf_gsat_walk", _c.c_int, [_ctx, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    ("pmf_gsat_probe_vec", _c.c_int, [_ctx, _c.c_void_p, _c.POINTER(_c.c_int32)]),
    ("pmf_gsat_get_volumes", _c.c_int, [_ctx, _c.c_void_p, _c.c_int64, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_double)]),
    ("pmf_gsat_get_d", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_greedy_select", _c.c_int, [_ctx, _c.c_int32, _c.c_int32, _c.c_void_p]),
    ("pmf_sivm_select", _c.c_int, [_ctx, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_void_p]),
    ("pmf_aa_get_beta", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_aa_rounds", _c.c_int, [_ctx, _c.POINTER(_c.c_int32)]),
    ("pmf_chnmf_hull", _c.c_int, [_ctx, _c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("pmf_chnmf_set_limits", _c.c_int, [_ctx, _c.c_int32, _c.c_int32]),
    ("pmf_chnmf_routes", _c.c_int, [_ctx, _c.c_void_p]),
    ("pmf_vq_columns", _c.c_int, [_ctx, _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_void_p]),
    ("pmf_vq_assign", _c.c_int, [_ctx, _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_void_p]),
    ("pmf_set_v_gather_f32", _c.c_int, [_ctx, _ctx, _c.c_void_p, _c.c_int64]),
    ("pmf_get_v_dense_f32", _c.c_int, [_ctx, _c.c_void_p, _c.c_int64]),
    ("pmf_svd_decompose", _c.c_int, [_ctx, _c.POINTER(_c.c_int32)]),
    ("pmf_svd_rank", _c.c_int, [_ctx, _c.POINTER(_c.c_int32)]),
    ("pmf_svd_get", _c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("pmf_cur_sqnorms", _c.c_int, [_ctx, _c.c_void_p, _c.c_void_p]),
    ("pmf_cur_compute", _c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_int32, _c.c_void_p, _c.c_void_p, _c.c_int32]),
    ("pmf_cur_get", _c.c_int, [_ctx, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("pmf_cur_ferr", _c.c_int, [_ctx, _c.POINTER(_c.c_double)]),
    ("pmf_cur_leverage", _c.c_int, [_ctx, _c.c_int32, _c.c_int32, _c.c_void_p, _c.c_void_p]),
    ("pmf_stream_begin", _c.c_int, [_ctx, _c.c_uint32, _c.c_int64]),
    ("pmf_stream_tile", _c.c_int, [_ctx, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_int64]),
    ("pmf_stream_end", _c.c_int, [_ctx, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int32)]),
    ("pmf_last_loop_ms", _c.c_int, [_ctx, _c.POINTER(_c.c_double)]),
    ("pmf_profile_enable", _c.c_int, [_ctx, _c.c_int32]),
    ("pmf_kernel_stats", _c.c_int, [_ctx, _c.POINTER(_c.c_char_p), _c.POINTER(_c.c_int64),
                                    _c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                                    _c.POINTER(_c.c_double)]),
    ("pmf_host_checksum", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("pmf_set_option", _c.c_int, [_ctx, _c.c_char_p, _c.c_int64]),
    ("pmf_set_host_allreduce", _c.c_int, [_ctx, _c.c_void_p, _c.c_void_p]),
    ("pmf_ipc_export", _c.c_int, [_ctx, _c.c_int32, _c.c_int32, _c.c_void_p]),
    ("pmf_ipc_import", _c.c_int, [_ctx, _c.c_void_p, _c.c_int32]),
    ("pmf_ipc_selftest", _c.c_int, [_ctx, _c.c_int32, _c.POINTER(_c.c_int32)]),
    ("pmf_collective_name", _c.c_char_p, [_ctx]),
    ("pmf_invalidate_v", _c.c_int, [_ctx]),
    ("pmf_snapshot_w", _c.c_int, [_ctx]),
    ("pmf_restore_w", _c.c_int, [_ctx]),
    ("pmf_snapshot_h", _c.c_int, [_ctx]),
    ("pmf_restore_h", _c.c_int, [_ctx]),
    ("pmf_collective_ms", _c.c_int, [_ctx, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64)]),
    ("pmf_kernel_exec_flops", _c.c_int, [_ctx, _c.POINTER(_c.c_double)]),
    ("pmf_kernel_launch_ms", _c.c_int, [_ctx, _c.c_void_p, _c.c_int64, _c.POINTER(_c.c_int64)]),
    ("pmf_nnqp_counters", _c.c_int, [_ctx, _c.POINTER(_c.c_int64), _c.c_int32]),
    ("pmf_synchronize", _c.c_int, [_ctx]),
    ("pmf_abort", _c.c_int, [_ctx, _c.c_int32]),
    ("pmf_path_name", _c.c_char_p, [_ctx]),
]

HOST_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32)

_lib = None


class PmfError(RuntimeError):
    """A negative status from libpymf_hip; `.code` is the PMF_E* value (include/pymf_hip.h)."""
    code = None


def load():
    """dlopen libpymf_hip.so and bind every declared symbol.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PmfError("libpymf_hip.so not built: run `python -m pymf_amd.csrc.build` "
                       "(hipcc, gfx950). There is no CPU fallback.")
    if not os.environ.get("PMF_LIB"):                 # (an A/B build named explicitly is the caller's business)
        from .csrc import build as _build
        if _build.built_hash() != _build.source_hash():
            raise PmfError("libpymf_hip.so was not built from the sources at hand (hash of csrc/*.h, csrc/*.hip, "
                           "include/pymf_hip.h and the flags differs from libpymf_hip.so.srchash): run "
                           "`python -m pymf_amd.csrc.build`. A stale binary is never loaded.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, ctx=None):
    if rc == PMF_ESINGULAR:                 # what the reference's np.linalg.inv raises (snmf.py:69)
        raise np.linalg.LinAlgError("Singular matrix")
    if rc != PMF_OK:
        msg = load().pmf_last_error(ctx)
        err = PmfError("libpymf_hip error %d: %s" % (rc, (msg or b"").decode("utf-8", "replace")))
        err.code = int(rc)
        raise err


def device_count():
    n = ctypes.c_int32(0)
    rc = load().pmf_device_count(ctypes.byref(n))
    if rc != PMF_OK:
        return 0
    return int(n.value)


def nccl_unique_id():
    buf = ctypes.create_string_buffer(NCCL_ID_BYTES)
    check(load().pmf_nccl_unique_id(buf))
    return buf.raw


def host_checksum(a):
    """(shape, dtype, 128-bit digest of the bytes) of a host array: the change detector of the host
    classes (pmf_host_checksum; runs without a GPU).  Non-contiguous input is digested through a
    contiguous copy."""
    a = np.asarray(a)
    c = a if a.flags.c_contiguous else np.ascontiguousarray(a)
    out = (ctypes.c_uint64 * 2)()
    check(load().pmf_host_checksum(c.ctypes.data if c.size else None, c.nbytes, out))
    return (a.shape, a.dtype.str, int(out[0]), int(out[1]))


def _f32c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def check_csc(m, n, indptr, indices):
    """pmf_check_csc: raises PmfError (code PMF_EINVAL) unless the arrays are the CSC image of an m x n matrix as
    pmf_set_v_csc_f32 takes it.  Runs on the host alone."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    if indptr.shape[0] != n + 1:
        raise ValueError("indptr must have n + 1 entries")
    check(load().pmf_check_csc(m, n, indptr.ctypes.data, indices.ctypes.data, int(indices.shape[0])))


def check_csr(m, n, indptr, indices):
    """pmf_check_csr: raises PmfError (code PMF_EINVAL) unless the arrays are the CSR image of an m x n matrix as
    pmf_set_v_csr_f32 takes it (unsorted rows and repeated entries are fine).  Runs on the host alone."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    if indptr.shape[0] != m + 1:
        raise ValueError("indptr must have m + 1 entries")
    check(load().pmf_check_csr(m, n, indptr.ctypes.data, indices.ctypes.data, int(indices.shape[0])))


class Context(object):
    """Thin owner of one pmf_ctx*."""

    def __init__(self, algo, m_local, n, k, device=0, rank=0, nranks=1, nccl_id=None):
        self._lib = load()
        self._h = ctypes.c_void_p()
        idbuf = ctypes.create_string_buffer(nccl_id, NCCL_ID_BYTES) if nccl_id else None
        check(self._lib.pmf_ctx_create(ctypes.byref(self._h), algo, m_local, n, k, device, rank,
                                       nranks, idbuf))
        self.m, self.n, self.k = int(m_local), int(n), int(k)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.pmf_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        check(rc, self._h)

    @property
    def path_name(self):
        return self._lib.pmf_path_name(self._h).decode()

    def set_v_dense(self, V):
        V = np.asarray(V)
        assert V.shape == (self.m, self.n)
        if V.dtype == np.float64 and V.flags.c_contiguous:       # rounded on the device: no host conversion pass
            self._chk(self._lib.pmf_set_v_dense_f64(self._h, V.ctypes.data, V.shape[1]))
            return
        if V.dtype != np.float32 or not V.flags.c_contiguous:
            V = _f32c(V)
        self._chk(self._lib.pmf_set_v_dense_f32(self._h, V.ctypes.data, V.shape[1]))

    def set_v_csr(self, indptr, indices, vals):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        vals = _f32c(vals)
        assert indptr.shape[0] == self.m + 1
        self._chk(self._lib.pmf_set_v_csr_f32(self._h, indptr.ctypes.data, indices.ctypes.data,
                                              vals.ctypes.data, int(vals.shape[0])))

    def set_v_csc(self, indptr, indices, vals):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        vals = _f32c(vals)
        assert indptr.shape[0] == self.n + 1 and indices.shape[0] == vals.shape[0]
        self._chk(self._lib.pmf_set_v_csc_f32(self._h, indptr.ctypes.data, indices.ctypes.data,
                                              vals.ctypes.data, int(vals.shape[0])))

    def fill_v_uniform(self, seed, row0=0):
        self._chk(self._lib.pmf_fill_v_uniform(self._h, seed, row0))

    def fill_w_uniform(self, seed, row0=0):
        self._chk(self._lib.pmf_fill_w_uniform(self._h, seed, row0))

    def fill_h_uniform(self, seed):
        self._chk(self._lib.pmf_fill_h_uniform(self._h, seed))

    def _set_factor(self, A, shape, f32_fn, f64_fn):
        A = np.asarray(A)
        assert A.shape == shape, (A.shape, shape)
        if A.dtype == np.float64 and A.flags.c_contiguous:       # the reference's default dtype: rounded on the device
            self._chk(f64_fn(self._h, A.ctypes.data))
        else:
            A = _f32c(A)
            self._chk(f32_fn(self._h, A.ctypes.data))

    def set_w(self, W):
        self._set_factor(W, (self.m, self.k), self._lib.pmf_set_w_f32, self._lib.pmf_set_w_f64)

    def set_h(self, H):
        self._set_factor(H, (self.k, self.n), self._lib.pmf_set_h_f32, self._lib.pmf_set_h_f64)

    def get_w(self):
        W = np.empty((self.m, self.k), dtype=np.float32)
        self._chk(self._lib.pmf_get_w_f32(self._h, W.ctypes.data))
        return W

    def get_h(self):
        H = np.empty((self.k, self.n), dtype=np.float32)
        self._chk(self._lib.pmf_get_h_f32(self._h, H.ctypes.data))
        return H

    def _get_into(self, out, shape, f32_fn, f64_fn):
        """Write a factor straight into the caller's array when that is a C-contiguous float32 / float64 array of the
        right shape (float64: widened on the device); returns False when it is not (the caller copies)."""
        if type(out) is not np.ndarray or out.shape != shape or not out.flags.c_contiguous or not out.flags.writeable:
            return False
        if out.dtype == np.float64:
            self._chk(f64_fn(self._h, out.ctypes.data))
        elif out.dtype == np.float32:
            self._chk(f32_fn(self._h, out.ctypes.data))
        else:
            return False
        return True

    def get_w_into(self, out):
        return self._get_into(out, (self.m, self.k), self._lib.pmf_get_w_f32, self._lib.pmf_get_w_f64)

    def get_h_into(self, out):
        return self._get_into(out, (self.k, self.n), self._lib.pmf_get_h_f32, self._lib.pmf_get_h_f64)

    def update_w(self):
        self._chk(self._lib.pmf_update_w(self._h))

    def update_h(self):
        self._chk(self._lib.pmf_update_h(self._h))

    def frobenius(self):
        out = ctypes.c_double(0.0)
        self._chk(self._lib.pmf_frobenius(self._h, ctypes.byref(out)))
        return float(out.value)

    def factorize(self, niter, compute_w=True, compute_h=True, compute_err=True, conv_eps=1e-8):
        """Returns (ferr ndarray or None, iters_done, converged_at)."""
        flags = (COMPUTE_W if compute_w else 0) | (COMPUTE_H if compute_h else 0) | \
                (COMPUTE_ERR if compute_err else 0)
        ferr = np.zeros(max(int(niter), 1), dtype=np.float64) if compute_err else None
        done = ctypes.c_int32(0)
        conv = ctypes.c_int32(-1)
        self._chk(self._lib.pmf_factorize(self._h, int(niter), flags, float(conv_eps),
                                          ferr.ctypes.data if compute_err else None,
                                          ctypes.byref(done), ctypes.byref(conv)))
        if compute_err:
            ferr = ferr[:int(niter)]
        return ferr, int(done.value), int(conv.value)

    def set_lambda(self, lamb_w, lamb_h):
        self._chk(self._lib.pmf_set_lambda(self._h, float(lamb_w), float(lamb_h)))

    def get_lambda(self):
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._chk(self._lib.pmf_get_lambda(self._h, ctypes.byref(a), ctypes.byref(b)))
        return float(a.value), float(b.value)

    def rnmf_update_s(self):
        self._chk(self._lib.pmf_rnmf_update_s(self._h))

    def rnmf_set_s(self, S):
        S = _f32c(S)
        assert S.shape == (self.m, self.n), (S.shape, self.m, self.n)
        self._chk(self._lib.pmf_rnmf_set_s_f32(self._h, S.ctypes.data))

    def rnmf_get_s(self):
        S = np.empty((self.m, self.n), dtype=np.float32)
        self._chk(self._lib.pmf_rnmf_get_s_f32(self._h, S.ctypes.data))
        return S

    def stream_begin(self, compute_w=True, compute_h=True, compute_err=True, max_tile_rows=65536, resid=False):
        """Open one streamed pass over V (pmf_stream_begin); resid=True: direct residual pass only."""
        flags = STREAM_RESID if resid else \
            ((COMPUTE_W if compute_w else 0) | (COMPUTE_H if compute_h else 0) | (COMPUTE_ERR if compute_err else 0))
        self._chk(self._lib.pmf_stream_begin(self._h, flags, int(max_tile_rows)))
        self._tiles_alive = []

    def stream_tile(self, row0, tile):
        """Hand rows [row0, row0 + len(tile)) to the pass; `tile` is kept alive until two tiles later."""
        t = np.ascontiguousarray(tile, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != self.n:
            raise ValueError("tile must be rows x %d" % self.n)
        self._chk(self._lib.pmf_stream_tile(self._h, int(row0), t.shape[0], t.ctypes.data, t.shape[1]))
        self._tiles_alive = (self._tiles_alive + [t])[-3:]

    def stream_end(self):
        """Close the pass: returns (ferr or None, needs_direct)."""
        ferr = ctypes.c_double(-1.0)
        nd = ctypes.c_int32(0)
        self._chk(self._lib.pmf_stream_end(self._h, ctypes.byref(ferr), ctypes.byref(nd)))
        self._tiles_alive = []
        return float(ferr.value), bool(nd.value)

    def nndsvd_init(self):
        """W, H <- NNDSVD of the resident V (pymf/nndsvd.py:79-106); returns the rank found."""
        found = ctypes.c_int32(0)
        self._chk(self._lib.pmf_nndsvd_init(self._h, ctypes.byref(found)))
        return int(found.value)

    def cnmf_init(self, sel, km_niter=10):
        """CNMF.init_h on the device (pmf_cnmf_init): k-means from the samples `sel` (sorted), then H, G (unless set) and
        W = V G (unless set).  Returns the cluster index of every sample."""
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        assert sel.shape == (self.k,), (sel.shape, self.k)
        out = np.empty(self.n, dtype=np.int32)
        self._chk(self._lib.pmf_cnmf_init(self._h, sel.ctypes.data, int(km_niter), out.ctypes.data))
        return out

    def set_g(self, G):
        G = np.ascontiguousarray(G, dtype=np.float64)
        assert G.shape == (self.n, self.k), (G.shape, self.n, self.k)
        self._chk(self._lib.pmf_set_g_f64(self._h, G.ctypes.data))

    def get_g(self):
        G = np.empty((self.n, self.k), dtype=np.float64)
        self._chk(self._lib.pmf_get_g_f64(self._h, G.ctypes.data))
        return G

    def get_assigned(self):
        """Kmeans: the cluster index of every sample (pmf_cluster_get_assigned)."""
        out = np.empty(self.n, dtype=np.int32)
        self._chk(self._lib.pmf_cluster_get_assigned(self._h, out.ctypes.data))
        return out

    def set_assigned(self, assigned):
        a = np.ascontiguousarray(assigned, dtype=np.int32)
        assert a.shape == (self.n,), (a.shape, self.n)
        self._chk(self._lib.pmf_cluster_set_assigned(self._h, a.ctypes.data))

    def get_select(self):
        """SIVM, GREEDY: the selected column indices of the last update_w, in selection order (pmf_sivm_get_select)."""
        out = np.empty(self.k, dtype=np.int32)
        self._chk(self._lib.pmf_sivm_get_select(self._h, out.ctypes.data))
        return out

    def get_volumes(self):
        """SIVM_SGREEDY: the num_bases - 1 volumes of the rounds of the last update_w, float64 (pmf_sivm_get_volumes)."""
        out = np.empty(max(self.k - 1, 1), dtype=np.float64)
        self._chk(self._lib.pmf_sivm_get_volumes(self._h, out.ctypes.data))
        return out[:self.k - 1]

    def gsat_start(self, select, force=False):
        """SIVM_GSAT: the walk's state from the context's W and `select` (pmf_gsat_start); True when a state was made, False
        when the one at hand belongs to the current W and was kept."""
        sel = np.ascontiguousarray(select, dtype=np.int32)
        assert sel.shape == (self.k,), (sel.shape, self.k)
        started = ctypes.c_int32(0)
        self._chk(self._lib.pmf_gsat_start(self._h, sel.ctypes.data, 1 if force else 0, ctypes.byref(started)))
        return bool(started.value)

    def gsat_walk(self, idx):
        """SIVM_GSAT: the probes `idx` (data columns) in order; per probe the vertex it replaced, -1 rejected, -2 skipped
        (pmf_gsat_walk)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        out = np.empty(max(idx.shape[0], 1), dtype=np.int32)
        self._chk(self._lib.pmf_gsat_walk(self._h, idx.ctypes.data, int(idx.shape[0]), out.ctypes.data))
        return out[:idx.shape[0]]

    def gsat_probe_vec(self, vec):
        """SIVM_GSAT: online_update_w on a vector of data_dimension values; the vertex it replaced or -1 (pmf_gsat_probe_vec)."""
        vec = _f32c(vec).reshape(-1)
        assert vec.shape == (self.m,), (vec.shape, self.m)
        slot = ctypes.c_int32(-1)
        self._chk(self._lib.pmf_gsat_probe_vec(self._h, vec.ctypes.data, ctypes.byref(slot)))
        return int(slot.value)

    def gsat_get_volumes(self):
        """SIVM_GSAT: (the reference's _v since the start as a float64 array, V) (pmf_gsat_get_volumes)."""
        count, V = ctypes.c_int64(0), ctypes.c_double(0.0)
        self._chk(self._lib.pmf_gsat_get_volumes(self._h, None, 0, ctypes.byref(count), ctypes.byref(V)))
        out = np.empty(max(int(count.value), 1), dtype=np.float64)
        self._chk(self._lib.pmf_gsat_get_volumes(self._h, out.ctypes.data, int(count.value), ctypes.byref(count), ctypes.byref(V)))
        return out[:int(count.value)], float(V.value)

    def gsat_get_d(self):
        """SIVM_GSAT: the reference's D, (num_bases + 1) x (num_bases + 1) float64 (pmf_gsat_get_d)."""
        D = np.empty((self.k + 1, self.k + 1), dtype=np.float64)
        self._chk(self._lib.pmf_gsat_get_d(self._h, D.ctypes.data))
        return D

    def greedy_select(self, nsel, transposed=False):
        """GREEDY / GREEDYCUR: `nsel` indices in selection order among the columns of the data, or (transposed) among its rows
        (pmf_greedy_select)."""
        out = np.empty(int(nsel), dtype=np.int32)
        self._chk(self._lib.pmf_greedy_select(self._h, 1 if transposed else 0, int(nsel), out.ctypes.data))
        return out

    def sivm_select(self, nsel, transposed=False, metric=0, init=0, path=0):
        """SIVM / SIVM_CUR: `nsel` indices in SIVM's selection order among the columns of the data, or (transposed) among its
        rows; metric 0 l2, 1 l1, 2 cosine; init 0 fastmap, 1 origin (the first entry is then -1); path 0 by shape, 1 the
        column-panel pass, 2 the long-sample pass (pmf_sivm_select)."""
        out = np.empty(max(int(nsel), 0), dtype=np.int32)
        self._chk(self._lib.pmf_sivm_select(self._h, 1 if transposed else 0, int(nsel), int(metric), int(init), int(path), out.ctypes.data))
        return out

    def get_beta(self):
        """AA: beta of the last update_w, num_bases x num_samples float64 (pmf_aa_get_beta)."""
        out = np.empty((self.k, self.n), dtype=np.float64)
        self._chk(self._lib.pmf_aa_get_beta(self._h, out.ctypes.data))
        return out

    def aa_rounds(self):
        """AA: rounds of pricing pass and master step the last update_w took (pmf_aa_rounds)."""
        r = ctypes.c_int32(0)
        self._chk(self._lib.pmf_aa_rounds(self._h, ctypes.byref(r)))
        return int(r.value)

    def chnmf_hull(self, R):
        """CHNMF: the ascending indices (int32) of the columns on the convex hulls of the pairwise projections by R, base_sel x
        data_dimension float64 (pmf_chnmf_hull); the context's data must be resident."""
        R = np.ascontiguousarray(R, dtype=np.float64)
        assert R.ndim == 2 and R.shape[1] == self.m, (R.shape, self.m)
        out = np.empty(self.n, dtype=np.int32)
        cnt = ctypes.c_int64(0)
        self._chk(self._lib.pmf_chnmf_hull(self._h, R.ctypes.data, int(R.shape[0]), out.ctypes.data, int(out.shape[0]), ctypes.byref(cnt)))
        return out[:int(cnt.value)].copy()

    def chnmf_set_limits(self, survivor_cap=0, max_wgs=0):
        """CHNMF: survivor capacity of the exact-hull kernel and workgroup cap of the sweeps, 0 = the build's (pmf_chnmf_set_limits)."""
        self._chk(self._lib.pmf_chnmf_set_limits(self._h, int(survivor_cap), int(max_wgs)))

    def chnmf_routes(self):
        """CHNMF: pairs of the last chnmf_hull by route: (32-direction filter, 128-direction rerun, host) (pmf_chnmf_routes)."""
        out = np.zeros(3, dtype=np.int32)
        self._chk(self._lib.pmf_chnmf_routes(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def vq_columns(self, Q, metric=0, want_dist=True):
        """The data column nearest to each column of Q (data_dimension x nq <= 128, float32; metric 0 l2, 1 l1), lowest
        column on ties: (int32 indices [nq], float64 distances [nq] or None) (pmf_vq_columns).  Any context with dense
        resident data."""
        Q = _f32c(Q)
        assert Q.ndim == 2 and Q.shape[0] == self.m, (Q.shape, self.m)
        nq = int(Q.shape[1])
        idx = np.empty(max(nq, 1), dtype=np.int32)
        dist = np.empty(max(nq, 1), dtype=np.float64) if want_dist else None
        self._chk(self._lib.pmf_vq_columns(self._h, Q.ctypes.data, nq, nq, int(metric), idx.ctypes.data,
                                           None if dist is None else dist.ctypes.data))
        return idx[:nq], (None if dist is None else dist[:nq])

    def vq_assign(self, Q, metric=0, want_idx=True, want_dist=False):
        """The column of Q (data_dimension x nq <= 128, float32) nearest to each data column, lowest on ties, and / or the
        whole nq x num_samples float64 distance block: (int32 [num_samples] or None, float64 [nq][num_samples] or None)
        (pmf_vq_assign).  Any context with dense resident data."""
        Q = _f32c(Q)
        assert Q.ndim == 2 and Q.shape[0] == self.m, (Q.shape, self.m)
        nq = int(Q.shape[1])
        idx = np.empty(self.n, dtype=np.int32) if want_idx else None
        dist = np.empty((max(nq, 1), self.n), dtype=np.float64) if want_dist else None
        self._chk(self._lib.pmf_vq_assign(self._h, Q.ctypes.data, nq, nq, int(metric), None if idx is None else idx.ctypes.data,
                                          None if dist is None else dist.ctypes.data))
        return idx, (None if dist is None else dist[:nq])

    def set_v_gather(self, src, idx=None):
        """This context's dense V <- src's resident V[:, idx] on the device (pmf_set_v_gather_f32); idx None: all of src's
        columns in order.  Indices may repeat and come in any order; src is a Context with dense resident data."""
        if idx is None:
            self._chk(self._lib.pmf_set_v_gather_f32(self._h, src._h, None, int(src.n)))
            return
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        self._chk(self._lib.pmf_set_v_gather_f32(self._h, src._h, idx.ctypes.data if idx.size else None, int(idx.shape[0])))

    def get_v_dense(self):
        """The resident dense V, m x n float32 (pmf_get_v_dense_f32)."""
        V = np.empty((self.m, self.n), dtype=np.float32)
        self._chk(self._lib.pmf_get_v_dense_f32(self._h, V.ctypes.data, V.shape[1]))
        return V

    def svd_decompose(self):
        """PCA / SVD: decompose the resident V (pmf_svd_decompose); returns the number of singular triples kept."""
        r = ctypes.c_int32(0)
        self._chk(self._lib.pmf_svd_decompose(self._h, ctypes.byref(r)))
        return int(r.value)

    def svd_rank(self):
        """PCA / SVD: the rank of the last decomposition of the resident V (pmf_svd_rank)."""
        r = ctypes.c_int32(0)
        self._chk(self._lib.pmf_svd_rank(self._h, ctypes.byref(r)))
        return int(r.value)

    def svd_get(self, rank, want="USV"):
        """PCA / SVD: U (m x rank), the singular values (rank) and V (rank x n) of the last decomposition, float64
        (pmf_svd_get); `rank` is what svd_decompose / svd_rank returned.  Factors not named in `want` come back as None."""
        U = np.zeros((self.m, rank), dtype=np.float64) if "U" in want else None
        S = np.zeros(rank, dtype=np.float64) if "S" in want else None
        V = np.zeros((rank, self.n), dtype=np.float64) if "V" in want else None
        self._chk(self._lib.pmf_svd_get(self._h, *(None if a is None else a.ctypes.data for a in (U, S, V))))
        return U, S, V

    def cur_sqnorms(self):
        """CUR / CMD: the row sums (m) and column sums (n) of data**2, float64 (pmf_cur_sqnorms)."""
        row, col = np.zeros(self.m, dtype=np.float64), np.zeros(self.n, dtype=np.float64)
        self._chk(self._lib.pmf_cur_sqnorms(self._h, row.ctypes.data, col.ctypes.data))
        return row, col

    def cur_leverage(self, k_rows, k_cols, want="rc"):
        """CURSL: the unnormalised leverage scores, float64 (pmf_cur_leverage): for the rows (m) the squared row norms of the
        leading min(k_rows, rank) left singular vectors, for the columns (n) the squared column norms of the leading
        min(k_cols, rank) right singular vectors.  A side not named in `want` ("r", "c") comes back as None."""
        row = np.zeros(self.m, dtype=np.float64) if "r" in want else None
        col = np.zeros(self.n, dtype=np.float64) if "c" in want else None
        self._chk(self._lib.pmf_cur_leverage(self._h, int(k_rows), int(k_cols), *(None if a is None else a.ctypes.data for a in (row, col))))
        return row, col

    def cur_compute(self, rid, rcnt, cid, ccnt):
        """CUR / CMD: computeUCR for the row indices `rid` with multiplicities `rcnt` and the column indices `cid` with
        `ccnt` (pmf_cur_compute); negative indices count from the end."""
        rid, rcnt, cid, ccnt = (np.ascontiguousarray(a, dtype=np.int32) for a in (rid, rcnt, cid, ccnt))
        assert rid.ndim == 1 and rid.shape == rcnt.shape and cid.ndim == 1 and cid.shape == ccnt.shape
        self._chk(self._lib.pmf_cur_compute(self._h, rid.ctypes.data, rcnt.ctypes.data, rid.shape[0],
                                            cid.ctypes.data, ccnt.ctypes.data, cid.shape[0]))
        self._cur_shape = (int(rid.shape[0]), int(cid.shape[0]))

    def cur_get(self, want="CUR"):
        """CUR / CMD: C (m x nc), U (nc x nr) and R (nr x n) of the last cur_compute, float64 (pmf_cur_get).  Factors not
        named in `want` come back as None."""
        nr, nc = self._cur_shape
        C = np.zeros((self.m, nc), dtype=np.float64) if "C" in want else None
        U = np.zeros((nc, nr), dtype=np.float64) if "U" in want else None
        R = np.zeros((nr, self.n), dtype=np.float64) if "R" in want else None
        self._chk(self._lib.pmf_cur_get(self._h, *(None if a is None else a.ctypes.data for a in (C, U, R))))
        return C, U, R

    def cur_ferr(self):
        """CUR / CMD on CSR data: ||data - C U R||_F of the last cur_compute from the trace identity, float64 (pmf_cur_ferr)."""
        out = ctypes.c_double(0.0)
        self._chk(self._lib.pmf_cur_ferr(self._h, ctypes.byref(out)))
        return float(out.value)

    def get_h64(self):
        H = np.empty((self.k, self.n), dtype=np.float64)
        self._chk(self._lib.pmf_get_h_f64(self._h, H.ctypes.data))
        return H

    def last_loop_ms(self):
        ms = ctypes.c_double(0.0)
        self._chk(self._lib.pmf_last_loop_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def profile_enable(self, on=True):
        self._chk(self._lib.pmf_profile_enable(self._h, 1 if on else 0))

    def kernel_stats(self):
        name = ctypes.c_char_p()
        n = ctypes.c_int64(0)
        ms = ctypes.c_double(0.0)
        fl = ctypes.c_double(0.0)
        by = ctypes.c_double(0.0)
        self._chk(self._lib.pmf_kernel_stats(self._h, ctypes.byref(name), ctypes.byref(n),
                                             ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)))
        ex = ctypes.c_double(0.0)
        self._chk(self._lib.pmf_kernel_exec_flops(self._h, ctypes.byref(ex)))
        return dict(name=(name.value or b"").decode(), launches=int(n.value), mean_ms=float(ms.value),
                    flops_per_launch=float(fl.value), bytes_per_launch=float(by.value),
                    executed_flops_per_launch=float(ex.value))

    def set_option(self, name, value):
        self._chk(self._lib.pmf_set_option(self._h, name.encode(), int(value)))

    def set_host_allreduce(self, reduce_array):
        """Route the cross-rank sums through `reduce_array(ndarray) -> ndarray` (the sum over all ranks)
        instead of RCCL: pmf_set_host_allreduce.  For plumbing checks with ranks that share one GPU."""
        def _cb(user, buf, count, is_f64):
            try:
                dt = np.float64 if is_f64 else np.float32
                a = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_double if is_f64 else ctypes.c_float)),
                                          shape=(int(count),))
                a[:] = np.asarray(reduce_array(a.copy()), dtype=dt)
                return 0
            except Exception:            # never let an exception cross the C boundary
                return 1
        self._host_ar_cb = HOST_ALLREDUCE_FN(_cb)      # keep the trampoline alive
        self._chk(self._lib.pmf_set_host_allreduce(self._h, ctypes.cast(self._host_ar_cb, ctypes.c_void_p), None))

    def ipc_export(self, rank, nranks):
        """This rank's IPC handle of its receive area (pmf_ipc_export), IPC_HANDLE_BYTES bytes."""
        buf = ctypes.create_string_buffer(IPC_HANDLE_BYTES)
        self._chk(self._lib.pmf_ipc_export(self._h, int(rank), int(nranks), buf))
        return buf.raw

    def ipc_import(self, handles):
        """Map the peers' receive areas: `handles` = every rank's handle in rank order (pmf_ipc_import)."""
        assert all(len(p_) == IPC_HANDLE_BYTES for p_ in handles)
        allh = ctypes.create_string_buffer(b"".join(handles), IPC_HANDLE_BYTES * len(handles))
        self._chk(self._lib.pmf_ipc_import(self._h, allh, len(handles)))

    def ipc_selftest(self, rounds=6):
        """True iff the one-shot all-reduce reproduced the other transport's sums `rounds` times (pmf_ipc_selftest)."""
        ok = ctypes.c_int32(0)
        self._chk(self._lib.pmf_ipc_selftest(self._h, int(rounds), ctypes.byref(ok)))
        return bool(ok.value)

    @property
    def collective_name(self):
        return (self._lib.pmf_collective_name(self._h) or b"").decode()

    def invalidate_v(self):
        self._chk(self._lib.pmf_invalidate_v(self._h))

    def snapshot_w(self):
        """Device-side copy of W before a step that may fail (pmf_snapshot_w)."""
        self._chk(self._lib.pmf_snapshot_w(self._h))

    def restore_w(self):
        self._chk(self._lib.pmf_restore_w(self._h))

    def snapshot_h(self):
        """Device-side copy of H and of the Gram state derived from it (pmf_snapshot_h)."""
        self._chk(self._lib.pmf_snapshot_h(self._h))

    def restore_h(self):
        self._chk(self._lib.pmf_restore_h(self._h))

    def kernel_launch_ms(self, cap=65536):
        """Durations (ms) of the dominant kernel's launches since profile_enable(), in launch order."""
        out = np.zeros(int(cap), dtype=np.float64)
        n = ctypes.c_int64(0)
        self._chk(self._lib.pmf_kernel_launch_ms(self._h, out.ctypes.data, int(cap), ctypes.byref(n)))
        return out[:min(int(n.value), int(cap))]

    def nnqp_counters(self, reset=False):
        """Live counts of k_nnqp_quad over the W half steps since the last reset (pmf_nnqp_counters)."""
        out = (ctypes.c_int64 * 8)()
        self._chk(self._lib.pmf_nnqp_counters(self._h, out, 1 if reset else 0))
        keys = ("wave_tasks", "passes", "sum_largest_system", "problems")
        return {"frame16": dict(zip(keys, (int(x) for x in out[0:4]))), "frame32": dict(zip(keys, (int(x) for x in out[4:8])))}

    def collective_ms(self):
        """(mean ms, count) of the per-iteration collective's launches since profile_enable() (pmf_collective_ms)."""
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        self._chk(self._lib.pmf_collective_ms(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def synchronize(self):
        self._chk(self._lib.pmf_synchronize(self._h))

    def abort(self, on=True):
        """Ask the running (or next) factorize() of this context to return early / clear the request (pmf_abort; the one
        call that may come from a second thread)."""
        self._chk(self._lib.pmf_abort(self._h, 1 if on else 0))
