// pmf_api.hip -- host side of libpymf_hip.so: the C ABI declared in include/pymf_hip.h.
//
// One pmf_ctx = one GPU, one HIP stream, optionally one RCCL communicator.
// Device layout (all float32, zero padded, row-major):
//   V  [mp][np]   mp = m rounded up to 64, np = n rounded up to 64
//   W  [mp][KP]   KP = 16*NT, NT in {1,2,4,8} (k <= 128)
//   H  [KP][np]
//   G  [KP][KP]   H H^T          PS [KP][np+KP]  (W^T V | W^T W)
// Zero padding is exactly neutral for all three update rules (a padded W column
// or H row/column stays 0 through every multiplicative step; SNMF/NMFALS put 1 on
// the padded diagonal of the k x k systems).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <atomic>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/pymf_hip.h"
#include "pmf_dev.h"
#include "pmf_ipc.h"
#include "pmf_small.h"
#include "pmf_tiled.h"
#include "pmf_fused_api.h"  // the one-pass kernels themselves: pmf_fused_tu.hip
#include "pmf_nnls_api.h"   // the sub-problem kernels themselves: pmf_nnls_tu.hip
#include "pmf_inv.h"
#include "pmf_csr.h"
#include "pmf_nmf_csr.h"
#include "pmf_nndsvd.h"
#include "pmf_topk.h"
#include "pmf_cnmf.h"
#include "pmf_cluster.h"
#include "pmf_sivm.h"
#include "pmf_colsel.h"
#include "pmf_sivm_csc.h"
#include "pmf_sgreedy.h"
#include "pmf_gsat.h"
#include "pmf_aa.h"
#include "pmf_chnmf.h"
#include "pmf_vq.h"
#include "pmf_gather.h"
#include "pmf_svd.h"
#include "pmf_cur.h"
#include "pmf_cur_csr.h"
#include "pmf_svd_csr.h"
#include "pmf_lev.h"
#include "pmf_greedy.h"
#include "pmf_greedy_csr.h"
#include "pmf_cluster_csr.h"

// the internal host code, by concern (each header: one anonymous-namespace block; the order is the dependency order)
#include "pmf_host_ctx.h"
#include "pmf_host_products.h"
#include "pmf_host_collective.h"
#include "pmf_host_nndsvd.h"
#include "pmf_host_nmf.h"
#include "pmf_host_snmf.h"
#include "pmf_host_nmf_csr.h"
#include "pmf_host_nmfals.h"
#include "pmf_host_transport.h"
#include "pmf_host_profile.h"
#include "pmf_host_loop.h"
#include "pmf_host_cnmf.h"
#include "pmf_host_cluster.h"
#include "pmf_host_sivm.h"
#include "pmf_host_colsel.h"
#include "pmf_host_sivm_csc.h"
#include "pmf_host_sgreedy.h"
#include "pmf_host_gsat.h"
#include "pmf_host_aa.h"
#include "pmf_host_chnmf.h"
#include "pmf_host_vq.h"
#include "pmf_host_gather.h"
#include "pmf_host_svd.h"
#include "pmf_host_cur_csr.h"
#include "pmf_host_svd_csr.h"
#include "pmf_host_cur.h"
#include "pmf_host_greedy_csr.h"
#include "pmf_host_cluster_csr.h"
#include "pmf_host_greedy.h"
#include "pmf_host_factorize.h"
#include "pmf_host_algos.h"

// =============================================================================================
extern "C" {

int pmf_device_count(int32_t* out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); *out = 0; return PMF_EHIP; }
  *out = n;
  return PMF_OK;
}

int pmf_nccl_unique_id(void* out) {
  static_assert(sizeof(ncclUniqueId) == PMF_NCCL_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) { g_create_error = ncclGetErrorString(r); return PMF_ENCCL; }
  std::memcpy(out, &id, sizeof(id));
  return PMF_OK;
}

int pmf_ctx_create(pmf_ctx** out, int32_t algo, int64_t m_local, int64_t n, int32_t k, int32_t device,
                   int32_t rank, int32_t nranks, const void* nccl_id) {
  if (!out) return fail(nullptr, PMF_EINVAL, "out is NULL");
  *out = nullptr;
  if (algo < 0 || algo >= kAlgoCount || !kAlgos[algo].family)
    return fail(nullptr, PMF_EINVAL, "algo must be 0 (NMF), 1 (NMFALS), 2 (SNMF), 3 (BNMF), 4 (RNMF), 5 (CNMF), 6 (Kmeans), 8 (Cmeans), 10 (SIVM), 11 (AA), 12 (PCA / SVD), 14 (CUR / CMD) or 15 (GREEDY)");
  if (m_local < 1 || n < 1 || k < 1) return fail(nullptr, PMF_EINVAL, "m, n, k must be >= 1");
  const AlgoRow& row = kAlgos[algo];
  if (const char* over = row.limits ? row.limits(m_local, n, k) : nullptr) return fail(nullptr, PMF_EINVAL, over);   // (the family's own limits before the general ones)
  if (row.one_rank && nranks > 1) return fail(nullptr, PMF_EINVAL, std::string(row.family) + ": one rank only in this build");
  // The reference has no limit on num_bases (nmf.py:116-120); the generic kernels beyond 128 bases have been checked against
  // the float64 oracles at 1 500, 2 304 and 2 432 bases (tests/sweeps/bigk_limit_probe.py, tests/test_gpu_bigk.py); beyond 2 432 (19 blocks of 128)
  // the 16-column block of H that k_nmf_h and k_trace_terms keep in LDS (64 bytes per basis) no longer fits the 160 KiB.  NMFALS /
  // NMFNNLS beyond 128 bases solve one variable at a time (k_nnqp_big) and stay at 1 024 (nmfals_limits).
  if (k > 2432) return fail(nullptr, PMF_EINVAL, "num_bases > 2432 is not supported by this build");
  if (n > (1 << 24)) return fail(nullptr, PMF_EINVAL, "n too large");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(nullptr, PMF_EINVAL, "bad rank/nranks");
  if (nranks > 1 && !nccl_id) return fail(nullptr, PMF_EINVAL, "nccl_id required when nranks > 1");
  pmf_ctx* c = new (std::nothrow) pmf_ctx();
  if (!c) return fail(nullptr, PMF_ENOMEM, "host allocation failed");
  c->algo = algo; c->m = m_local; c->n = n; c->k = k; c->device = device; c->rank = rank; c->nranks = nranks;
  const bool cluster = is_cluster(c);   // (no n-sized product buffers: pmf_cluster.h has its own)
  c->mp = round_up(m_local, 64);
  c->np = (int)round_up(n, 64);
  c->NT = k <= 16 ? 1 : k <= 32 ? 2 : k <= 64 ? 4 : 8;
  c->KP = 16 * c->NT;
  if (k > 128) {                // blocks of 128 bases on the NT = 8 tiled kernels (bigk_* below)
    c->nb = (int)((k + 127) / 128);
    c->KP = 128 * c->nb;
  }
  // 448 columns are not a panel count the wide (two waves per block) fused kernel takes: pad to 512
  if ((algo == PMF_ALGO_NMF || algo == PMF_ALGO_BNMF) && c->NT <= 2 && c->np == 448) c->np = 512;
  // ... and the cooperative kernel (pmf_coop.h) takes 6, 8, 12 or 16 column panels beyond 4
  if ((algo == PMF_ALGO_NMF || algo == PMF_ALGO_BNMF) && c->nb == 1 && k <= 128) {
    const int padded = pmf_coop_pad_np(c->NT, c->np);
    if (padded > 0) c->np = padded;
  }
  int rc = [&]() -> int {
    HIPCHK(c, hipSetDevice(device));
    HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreate(&c->ev0));
    HIPCHK(c, hipEventCreate(&c->ev1));
    if (nccl_id) {   // nranks == 1 with an id: a 1-rank communicator (exercises the RCCL path)
      ncclUniqueId id;
      std::memcpy(&id, nccl_id, sizeof(id));
      NCCLCHK(c, ncclCommInitRank(&c->comm, nranks, id, rank));
    }
    // partial-slab geometry for the tiled W^T V path: ~1024 row chunks over the grid
    const int n_panels = (c->np + 255) / 256;
    int want = std::max(1, 1024 / n_panels);
    int64_t blocks16 = c->mp / 16;
    c->nchunks = (int)std::min<int64_t>(want, blocks16);
    c->rows_per_chunk = (int)(round_up((blocks16 + c->nchunks - 1) / c->nchunks, 4) * 16);   // whole 64-row stages (k_colgemm_stream)
    c->nchunks = (int)((c->mp + c->rows_per_chunk - 1) / c->rows_per_chunk);
    c->fused_wgs = (c->nb == 1 && (algo == PMF_ALGO_NMF || algo == PMF_ALGO_SNMF || algo == PMF_ALGO_BNMF || algo == PMF_ALGO_RNMF))
                       ? pmf_fused_grid_for(c->NT, c->np, c->mp, /*allow_split=*/algo != PMF_ALGO_SNMF) : 0;
    {
      int bt = 0, rb = 0, pn = 0;
      if (c->fused_wgs == 0 && c->nb == 1 && pmf_coop_shape(c->NT, c->np, &bt, &rb, &pn) &&
          (algo == PMF_ALGO_NMF || algo == PMF_ALGO_BNMF || (algo == PMF_ALGO_RNMF && bt == 2 && rb == 4))) {
        c->fused8 = true;
        c->coop_bt = bt; c->coop_rb = rb;
        c->fused_wgs = pmf_coop_grid_for(c->mp, rb);
      }
    }
    const int nslabs = std::max(c->nchunks, c->fused_wgs);
    // dV [mp][np] is allocated by the first pmf_set_v_dense_f32 / pmf_fill_v_uniform: CSR and
    // streamed (pmf_stream_*) contexts never hold a dense V
    // (a PCA / SVD context allocates its row-count sized float32 buffers -- dW, dW1, dW2 -- with the first dense data or
    // float32-path W: ensure_wbufs.  On CSR data they are never read, and each is the size of the dense image)
    if (algo != PMF_ALGO_PCA) PMFCHK(dalloc(c, &c->dW, (size_t)c->mp * c->KP));
    PMFCHK(dalloc(c, &c->dH, (size_t)c->KP * c->np));
    PMFCHK(dalloc(c, &c->dG, (size_t)c->KP * c->KP));
    PMFCHK(dalloc(c, &c->dGd, (size_t)c->KP * c->KP));
    if (!cluster) PMFCHK(dalloc(c, &c->dPS, (size_t)ps_elems(c)));
    if (cluster) {
      PMFCHK(cluster_alloc(c));
    } else if (c->nb == 1) {
      PMFCHK(dalloc(c, &c->dSlab, (size_t)nslabs * ps_elems(c)));
    } else {                    // one 128-base block at a time: [chunk][128][max(np, KP) + 128]
      PMFCHK(dalloc(c, &c->dSlab, (size_t)c->nchunks * 128 * (std::max(c->np, c->KP) + 128)));
      if (algo != PMF_ALGO_PCA) {
        PMFCHK(dalloc(c, &c->dW1, (size_t)std::max<int64_t>(c->mp, c->np) * c->KP));
        PMFCHK(dalloc(c, &c->dW2, (size_t)c->mp * c->KP));
      }
    }
    c->dpart_cap = std::max<int64_t>(std::max<int64_t>(c->mp / 64, 1024), c->np / 8 + 2);
    PMFCHK(dalloc(c, &c->dPart, (size_t)c->dpart_cap));
    PMFCHK(dalloc(c, &c->dScal, 8));
    PMFCHK(dalloc(c, &c->dGpart, (size_t)PMF_HGRAM_MAX_WGS * c->KP * c->KP));
    PMFCHK(dalloc(c, &c->dT1part, (size_t)2 * PMF_HGRAM_MAX_WGS));
    PMFCHK(dalloc(c, &c->dTicket, 1));
    PMFCHK(dalloc(c, &c->dStop, 2));
    c->ferr_cap = 4096;
    PMFCHK(dalloc(c, &c->dFerr, (size_t)c->ferr_cap));
    if (algo == PMF_ALGO_RNMF) PMFCHK(dalloc(c, &c->dD, (size_t)c->mp * c->np));
    if (algo != PMF_ALGO_NMF && algo != PMF_ALGO_CNMF && !cluster) {
      if (!c->dW1 && algo != PMF_ALGO_PCA) PMFCHK(dalloc(c, &c->dW1, (size_t)std::max<int64_t>(c->mp, c->np) * c->KP));
      PMFCHK(dalloc(c, &c->dGinvT, (size_t)c->KP * c->KP));
    }
    if (algo == PMF_ALGO_SNMF) {
      PMFCHK(dalloc(c, &c->dMT, (size_t)c->KP * c->np));
      PMFCHK(dalloc(c, &c->dGinvD, (size_t)c->KP * c->KP));
    }
    if (algo == PMF_ALGO_CNMF) {
      PMFCHK(dalloc(c, &c->dMT, (size_t)c->KP * c->np));   // float32 G^T: the operand of W = V G (materialize_w)
      PMFCHK(cnmf_alloc(c));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PMF_OK;
  }();
  if (rc != PMF_OK) {
    g_create_error = c->err;
    pmf_ctx_destroy(c);
    return rc;
  }
  if (c->fused8) {
    char nb_[64];
    snprintf(nb_, sizeof(nb_), "k_nmf_coop<%d,%d,%d%s>", c->coop_bt, c->coop_rb, c->np / 64,
             algo == PMF_ALGO_BNMF ? ",bnmf" : algo == PMF_ALGO_RNMF ? ",rnmf" : "");
    c->path = nb_;
  } else
  c->path = (c->fused_wgs > 0) ? std::string(pmf_fused_kernel_name(c->NT, c->np, algo == PMF_ALGO_SNMF   ? FUSED_SNMF
                                                                           : algo == PMF_ALGO_BNMF ? FUSED_BNMF
                                                                           : algo == PMF_ALGO_RNMF ? FUSED_RNMF
                                                                                                   : FUSED_NMF))
                               : std::string("tiled");
  if (row.path) c->path = row.path;
  choose_stat_site(c, false);
  *out = c;
  return PMF_OK;
}

int pmf_ctx_destroy(pmf_ctx* c) {
  if (!c) return PMF_OK;
  (void)hipSetDevice(c->device);   // teardown: there is nobody to report a failing release to
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) (void)ncclCommDestroy(c->comm);
  if (c->ipc_exported) {
    for (int r = 0; r < PMF_IPC_MAX_RANKS; ++r)
      if (r != c->ipc.me && c->ipc.area[r]) (void)hipIpcCloseMemHandle(c->ipc.area[r]);
    if (c->ipc.area[c->ipc.me]) (void)hipFree(c->ipc.area[c->ipc.me]);
  }
  for (void* p : c->owned) (void)hipFree(p);
  for (hipEvent_t e : {c->ev_copied[0], c->ev_copied[1], c->ev_consumed[0], c->ev_consumed[1]})
    if (e) (void)hipEventDestroy(e);
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->w_stream) { (void)hipStreamSynchronize(c->w_stream); (void)hipStreamDestroy(c->w_stream); }
  for (hipEvent_t e : {c->ev_mt[0], c->ev_mt[1], c->ev_w[0], c->ev_w[1]}) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_ga) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->stat.ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->coll_ev) (void)hipEventDestroy(e);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return PMF_OK;
}

const char* pmf_last_error(const pmf_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }
const char* pmf_path_name(const pmf_ctx* c) { return c ? c->path.c_str() : ""; }

// RNMF keeps D = S - data on the device (rnmf.py:102,111); the reference's S is an attribute that SURVIVES new data
// (update_w / update_h then work on S - new data until the next update_s): around a change of V the state goes
// D -> S = D + V_old -> D = S - V_new.
static int rnmf_data_change_begin(pmf_ctx* c) {
  if (c->algo != PMF_ALGO_RNMF || !c->s_valid || !c->have_v || !c->dD || !c->dV) return PMF_OK;
  const int64_t E = c->mp * c->np;
  hipLaunchKernelGGL(k_acc_f32, dim3(elem_grid(E / 4)), dim3(256), 0, c->stream, c->dD, c->dV, E);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}
static int rnmf_data_change_end(pmf_ctx* c) {
  if (c->algo != PMF_ALGO_RNMF || !c->s_valid || !c->dD || !c->dV) return PMF_OK;
  const int64_t E = c->mp * c->np;
  hipLaunchKernelGGL(k_sub_f32, dim3(elem_grid(E / 4)), dim3(256), 0, c->stream, c->dD, c->dV, E);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// A dense fill of dV in two halves around the fill itself (a host upload, pmf_fill_v_uniform, pmf_set_v_gather_f32).
// dense_v_begin: whatever other form of the data the context held goes, dV exists, RNMF's D is S again.
static int dense_v_begin(pmf_ctx* c) {
  PMFCHK(sivm_csc_left(c));
  PMFCHK(cur_csr_left(c));
  PMFCHK(svd_csr_left(c));
  PMFCHK(greedy_csr_left(c));
  PMFCHK(cluster_csr_left(c));
  PMFCHK(ensure_wbufs(c));
  PMFCHK(ensure_dv(c));
  PMFCHK(rnmf_data_change_begin(c));
  return PMF_OK;
}
// dense_v_end: everything that follows a new V, the same whoever filled it
static int dense_v_end(pmf_ctx* c) {
  PMFCHK(rnmf_data_change_end(c));
  c->have_v = true; c->v_csr = false; c->csr_dense = false; v_replaced(c);
  nmf_csr_left(c);
  PMFCHK(local_vnorm(c));
  return PMF_OK;
}

static int set_v_dense(pmf_ctx* c, const void* V, bool f64, int64_t ld, const char* who) {
  if (!c || !V || ld < c->n) return fail(c, PMF_EINVAL, std::string(who) + ": bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  PMFCHK(dense_v_begin(c));
  PMFCHK(f64 ? upload_rows(c, c->dV, c->np, static_cast<const double*>(V), ld, c->m, c->n)
             : upload_rows(c, c->dV, c->np, static_cast<const float*>(V), ld, c->m, c->n));
  return dense_v_end(c);
}
int pmf_set_v_dense_f32(pmf_ctx* c, const float* V, int64_t ld) { return set_v_dense(c, V, false, ld, "pmf_set_v_dense_f32"); }
int pmf_set_v_dense_f64(pmf_ctx* c, const double* V, int64_t ld) { return set_v_dense(c, V, true, ld, "pmf_set_v_dense_f64"); }

int pmf_set_v_gather_f32(pmf_ctx* dst, pmf_ctx* src, const int64_t* idx, int64_t nsel) {
  if (!dst) return fail(nullptr, PMF_EINVAL, "pmf_set_v_gather_f32: dst is NULL");
  std::vector<int32_t> idx32;
  PMFCHK(gather_check(dst, src, idx, nsel, &idx32));     // every refusal: dst is as it was
  dst->hd_synced = false; dst->psd_fresh = false;        // (a new API call, as need() notes it)
  HIPCHK(dst, hipSetDevice(dst->device));
  PMFCHK(gather_stage_idx(dst, idx32));
  PMFCHK(dense_v_begin(dst));
  PMFCHK(gather_fill(dst, src, /*ident=*/idx == nullptr, nsel));
  return dense_v_end(dst);
}

int pmf_get_v_dense_f32(pmf_ctx* c, float* out, int64_t ld) {
  if (!c) return PMF_EINVAL;
  c->hd_synced = false; c->psd_fresh = false;
  if (const char* why = gather_no_dense(c)) return fail(c, PMF_EINVAL, std::string("pmf_get_v_dense_f32: the context ") + why);
  if (!out || ld < c->n) return fail(c, PMF_EINVAL, "pmf_get_v_dense_f32: out is NULL or ld < n");
  HIPCHK(c, hipSetDevice(c->device));
  return download_padded(c, out, ld, c->dV, c->np, c->m, c->n);
}

int pmf_set_v_csr_f32(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals,
                      int64_t nnz) {
  if (!c || !indptr || (nnz > 0 && (!indices || !vals)) || nnz < 0)
    return fail(c, PMF_EINVAL, "pmf_set_v_csr_f32: bad arguments");
  if (c->algo == PMF_ALGO_NMF) return nmf_csr_set_v(c, indptr, indices, vals, nnz);
  if (c->algo == PMF_ALGO_CUR) return cur_csr_set_v(c, indptr, indices, vals, nnz);
  if (c->algo == PMF_ALGO_PCA) return svd_csr_set_v(c, indptr, indices, vals, nnz);
  if (c->algo == PMF_ALGO_GREEDY) return greedy_csr_set_v(c, indptr, indices, vals, nnz);
  if (is_cluster(c)) return cluster_csr_set_v(c, indptr, indices, vals, nnz);
  if (c->algo != PMF_ALGO_SNMF) return fail(c, PMF_EINVAL, "CSR input is only wired for SNMF, NMF, CUR / CMD, PCA / SVD, GREEDY and Kmeans / Cmeans");
  // refused arrays never reach the device: what is resident stays as it was
  if (const char* why = csr_check(c->m, c->n, indptr, indices, nnz)) return fail(c, PMF_EINVAL, std::string("pmf_set_v_csr_f32: ") + why);
  HIPCHK(c, hipSetDevice(c->device));
  PMFCHK(dgrow(c, &c->dIndptr, (size_t)c->mp + 1));
  PMFCHK(dgrow(c, &c->dIndices, (size_t)nnz));
  PMFCHK(dgrow(c, &c->dVals, (size_t)nnz));
  std::vector<int64_t> ip((size_t)c->mp + 1);
  for (int64_t r = 0; r <= c->mp; ++r) ip[(size_t)r] = indptr[std::min(r, c->m)];
  HIPCHK(c, hipMemcpyAsync(c->dIndptr, ip.data(), ip.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  if (nnz) {
    HIPCHK(c, hipMemcpyAsync(c->dIndices, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dVals, vals, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->nnz = nnz; c->have_v = true; c->v_csr = true; c->csr_dense = false;
  v_replaced(c);                 // (V^T V for the Gram-space loop is formed on first use: k_csr_gram)
  // num_bases > 128: no CSR kernel at that width; n * num_bases beyond the 160 KiB LDS accumulator of the CSR scatter
  // (k_csr_p: e.g. 520 columns x 100 bases): no CSR kernel at that SIZE -- the rows are expanded once
  if (c->nb > 1 || (size_t)c->np * c->KP * sizeof(float) > (size_t)160 * 1024) {
    PMFCHK(ensure_dv(c));
    HIPCHK(c, hipMemsetAsync(c->dV, 0, (size_t)c->mp * c->np * sizeof(float), c->stream));
    hipLaunchKernelGGL(k_csr_densify, dim3((unsigned)((c->m + 255) / 256)), dim3(256), 0, c->stream, c->dIndptr, c->dIndices,
                       c->dVals, c->m, c->np, c->dV);
    HIPCHK(c, hipGetLastError());
    c->csr_dense = true;
    PMFCHK(local_vnorm(c));
  }
  return PMF_OK;
}

int pmf_check_csr(int64_t m, int64_t n, const int64_t* indptr, const int32_t* indices, int64_t nnz) {
  if (m < 1 || n < 1 || !indptr || (nnz > 0 && !indices) || nnz < 0) return fail(nullptr, PMF_EINVAL, "pmf_check_csr: bad arguments");
  if (const char* why = csr_check(m, n, indptr, indices, nnz)) return fail(nullptr, PMF_EINVAL, std::string("pmf_check_csr: ") + why);
  return PMF_OK;
}

int pmf_set_v_csc_f32(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz) {
  if (!c || !indptr || (nnz > 0 && (!indices || !vals)) || nnz < 0) return fail(c, PMF_EINVAL, "pmf_set_v_csc_f32: bad arguments");
  return sivm_csc_set_v(c, indptr, indices, vals, nnz);
}

int pmf_check_csc(int64_t m, int64_t n, const int64_t* indptr, const int32_t* indices, int64_t nnz) {
  if (m < 1 || n < 1 || !indptr || (nnz > 0 && !indices) || nnz < 0) return fail(nullptr, PMF_EINVAL, "pmf_check_csc: bad arguments");
  if (const char* why = csc_check(m, n, indptr, indices, nnz)) return fail(nullptr, PMF_EINVAL, std::string("pmf_check_csc: ") + why);
  return PMF_OK;
}

static int fill(pmf_ctx* c, float* X, int64_t ld, int64_t rows, int64_t cols, int64_t row0, uint64_t seed) {
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t E = rows * cols;
  hipLaunchKernelGGL(k_fill_uniform, dim3(elem_grid(E)), dim3(256), 0, c->stream, X, ld,
                     rows, cols, row0, cols, seed);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

int pmf_fill_v_uniform(pmf_ctx* c, uint64_t seed, int64_t row0) {
  if (!c) return PMF_EINVAL;
  PMFCHK(dense_v_begin(c));
  PMFCHK(fill(c, c->dV, c->np, c->m, c->n, row0, seed));
  return dense_v_end(c);
}
int pmf_fill_w_uniform(pmf_ctx* c, uint64_t seed, int64_t row0) {
  if (!c) return PMF_EINVAL;
  PMFCHK(svd_csr_refuse(c, "pmf_fill_w_uniform"));
  PMFCHK(greedy_csr_refuse(c, "pmf_fill_w_uniform"));
  PMFCHK(cluster_csr_refuse(c, "pmf_fill_w_uniform"));
  PMFCHK(ensure_wbufs(c));
  PMFCHK(w_pipe_join(c));        // (a pipelined W = V M write still in flight on the side stream must not land on the new W)
  PMFCHK(fill(c, c->dW, c->KP, c->m, c->k, row0, seed));
  w_replaced(c, /*by_caller=*/true);
  return PMF_OK;
}
int pmf_fill_h_uniform(pmf_ctx* c, uint64_t seed) {
  if (!c) return PMF_EINVAL;
  PMFCHK(svd_csr_refuse(c, "pmf_fill_h_uniform"));
  PMFCHK(greedy_csr_refuse(c, "pmf_fill_h_uniform"));
  PMFCHK(cluster_csr_refuse(c, "pmf_fill_h_uniform"));
  PMFCHK(fill(c, c->dH, c->np, c->k, c->n, 0, seed));
  h_replaced(c, false, true);
  return PMF_OK;
}

// The padding of W ([mp][KP]) and H ([KP][np]) is zero by construction and stays zero under every update
// rule -- unless a factor went non-finite (0 * nan = nan), e.g. behind a singular H H^T.  A fresh factor
// from the host therefore comes with fresh padding.
static int zero_padding(pmf_ctx* c, float* buf, int64_t ld, int64_t rows_total, int64_t rows_valid, int64_t cols_valid) {
  if (ld > cols_valid && rows_valid > 0)
    HIPCHK(c, hipMemset2DAsync(buf + cols_valid, (size_t)ld * sizeof(float), 0, (size_t)(ld - cols_valid) * sizeof(float),
                               (size_t)rows_valid, c->stream));
  if (rows_total > rows_valid)
    HIPCHK(c, hipMemsetAsync(buf + rows_valid * ld, 0, (size_t)(rows_total - rows_valid) * ld * sizeof(float), c->stream));
  return PMF_OK;
}

static int set_w(pmf_ctx* c, const void* W, bool f64, const char* who) {
  if (!c || !W) return fail(c, PMF_EINVAL, std::string(who) + ": bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  if (svd_csr(c)) return svd_csr_set_w(c, W, f64);
  PMFCHK(ensure_wbufs(c));
  PMFCHK(w_pipe_join(c));
  PMFCHK(zero_padding(c, c->dW, c->KP, c->mp, c->m, c->k));
  PMFCHK(f64 ? upload_rows(c, c->dW, c->KP, static_cast<const double*>(W), c->k, c->m, c->k)
             : upload_rows(c, c->dW, c->KP, static_cast<const float*>(W), c->k, c->m, c->k));
  w_replaced(c, /*by_caller=*/true);
  return PMF_OK;
}
int pmf_set_w_f32(pmf_ctx* c, const float* W) { return set_w(c, W, false, "pmf_set_w_f32"); }
int pmf_set_w_f64(pmf_ctx* c, const double* W) { return set_w(c, W, true, "pmf_set_w_f64"); }
int pmf_get_w_f64(pmf_ctx* c, double* W) {
  PMFCHK(need(c, false, true, false));
  if (!W) return fail(c, PMF_EINVAL, "W is NULL");
  if (svd_csr(c)) return svd_csr_get_w(c, W);
  PMFCHK(materialize_w(c));
  return download_rows<double>(c, W, c->dW, c->KP, c->m, c->k);
}
int pmf_set_h_f64(pmf_ctx* c, const double* H) {
  if (!c || !H) return fail(c, PMF_EINVAL, "pmf_set_h_f64: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  if (svd_csr(c)) return svd_csr_set_h(c, H, true);
  if (cluster_csr(c)) return cluster_csr_set_h(c, H);
  PMFCHK(zero_padding(c, c->dH, c->np, c->KP, c->k, c->n));
  PMFCHK(upload_rows<double>(c, c->dH, c->np, H, c->n, c->k, c->n));
  h_replaced(c, false, true);      // (here already: if the float64 copy below fails, Hd is widened anew from this H)
  if (h_in_f64(c)) {               // SNMF: the caller's float64 H as it is (nmf.py:120 keeps H in float64), beside its rounding
    if (!c->dHd) { PMFCHK(dalloc(c, &c->dHd, (size_t)c->KP * c->np)); PMFCHK(dalloc(c, &c->dSd, (size_t)c->KP * c->KP)); }
    const size_t bytes = (size_t)c->k * c->n * sizeof(double);
    PMFCHK(stage_reserve(c, bytes));
    HIPCHK(c, hipMemsetAsync(c->dHd, 0, (size_t)c->KP * c->np * sizeof(double), c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dStage, H, bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_unpack_rows_f64, dim3((unsigned)std::min<int64_t>(((int64_t)c->k * c->np + 255) / 256, 1024)), dim3(256), 0, c->stream,
                       reinterpret_cast<const double*>(c->dStage), (int64_t)c->k, (int64_t)c->n, c->dHd, (int64_t)c->np);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    h_replaced(c, false, false);     // (Hd holds the caller's float64 values, dH their rounding)
  }
  return PMF_OK;
}
int pmf_get_h_f64(pmf_ctx* c, double* H) {
  PMFCHK(need(c, false, false, true));
  if (!H) return fail(c, PMF_EINVAL, "H is NULL");
  if (svd_csr(c)) return svd_csr_get_h(c, H);
  if (greedy_csr(c) && c->gr_ht_valid) return greedy_csr_get_h(c, H);
  if (cluster_csr(c)) return cluster_csr_get_h(c, H);
  PMFCHK(nmf_csr_sync_h(c));
  if (h_in_f64(c) && c->dHd) {     // SNMF: the float64 H the device iterates on (entries another writer of the float32 H replaced: widened)
    PMFCHK(ensure_hd(c));
    const size_t bytes = (size_t)c->k * c->n * sizeof(double);
    PMFCHK(stage_reserve(c, bytes));
    hipLaunchKernelGGL(k_pack_rows_f64, dim3((unsigned)std::min<int64_t>(((int64_t)c->k * c->n + 255) / 256, 1024)), dim3(256), 0, c->stream,
                       (const double*)c->dHd, (int64_t)c->np, (int64_t)c->k, (int64_t)c->n, reinterpret_cast<double*>(c->dStage));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(H, c->dStage, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PMF_OK;
  }
  return download_rows<double>(c, H, c->dH, c->np, c->k, c->n);
}
int pmf_get_w_f32(pmf_ctx* c, float* W) {
  PMFCHK(need(c, false, true, false));
  if (!W) return fail(c, PMF_EINVAL, "W is NULL");
  if (svd_csr(c)) return svd_csr_get_w(c, W);
  PMFCHK(materialize_w(c));
  return download_padded(c, W, c->k, c->dW, c->KP, c->m, c->k);
}
int pmf_set_h_f32(pmf_ctx* c, const float* H) {
  if (!c || !H) return fail(c, PMF_EINVAL, "pmf_set_h_f32: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  if (svd_csr(c)) return svd_csr_set_h(c, H, false);
  if (cluster_csr(c)) return cluster_csr_set_h(c, H);
  PMFCHK(zero_padding(c, c->dH, c->np, c->KP, c->k, c->n));
  PMFCHK(upload_padded(c, c->dH, c->np, H, c->n, c->k, c->n));
  h_replaced(c, false, true);
  return PMF_OK;
}
int pmf_get_h_f32(pmf_ctx* c, float* H) {
  PMFCHK(need(c, false, false, true));
  if (!H) return fail(c, PMF_EINVAL, "H is NULL");
  if (svd_csr(c)) return svd_csr_get_h(c, H);
  if (greedy_csr(c) && c->gr_ht_valid) return greedy_csr_get_h(c, H);
  if (cluster_csr(c)) return cluster_csr_get_h(c, H);
  PMFCHK(nmf_csr_sync_h(c));
  return download_padded(c, H, c->n, c->dH, c->np, c->k, c->n);
}

// pmf_update_w / pmf_update_h: the family's step (kAlgos), with what it reads checked first
static int run_step(pmf_ctx* c, bool w_step) {
  if (!c) return PMF_EINVAL;
  if (c->algo == PMF_ALGO_CNMF) return PMF_OK;   // cnmf.py:70-76: both hooks are no-ops (the updates live in factorize)
  const AlgoRow& a = algo_row(c);
  int (*step)(pmf_ctx*) = w_step ? a.update_w : a.update_h;
  if (!step) return refuse_step(c, w_step ? "W step" : "H step");
  const Operands r = w_step ? a.reads_w : a.reads_h;
  PMFCHK(need(c, r.v, r.w, r.h));
  if (c->v_csr && (w_step ? a.dense_w : a.dense_h)) return fail(c, PMF_EINVAL, std::string(a.family) + ": dense data only");
  PMFCHK(step(c));
  PMFCHK(nmf_csr_sync_h(c));                     // (NMF on CSR data: dH follows the working copy H^T before the call returns)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!a.nmf_family) return PMF_OK;
  PMFCHK(ipc_check(c));                          // the NMF family: the exchange's verdict, and the inverse's behind a W step
  return w_step ? check_singular(c) : PMF_OK;
}
int pmf_update_w(pmf_ctx* c) { return run_step(c, true); }
int pmf_update_h(pmf_ctx* c) { return run_step(c, false); }
int pmf_frobenius(pmf_ctx* c, double* out) {
  PMFCHK(cur_csr_refuse(c, "pmf_frobenius"));
  PMFCHK(need(c, true, true, true));
  if (!out) return fail(c, PMF_EINVAL, "out is NULL");
  return algo_row(c).frobenius(c, out);
}

int pmf_factorize(pmf_ctx* c, int32_t niter, uint32_t flags, double conv_eps, double* ferr,
                  int32_t* iters_done, int32_t* converged_at) {
  const bool cw = flags & PMF_COMPUTE_W, ch = flags & PMF_COMPUTE_H, ce = flags & PMF_COMPUTE_ERR;
  if (!c) return PMF_EINVAL;
  PMFCHK(cur_csr_refuse(c, ce ? "pmf_factorize with PMF_COMPUTE_ERR" : "pmf_factorize"));
  const AlgoRow& a = algo_row(c);
  if (a.instead) return refuse_step(c, "iteration");
  const Operands r = a.loop_reads(cw, ch);
  PMFCHK(need(c, r.v, r.w, r.h));
  if (niter < 0 || (ce && !ferr)) return fail(c, PMF_EINVAL, "pmf_factorize: bad arguments");
  if (ce && c->v_csc) return fail(c, PMF_EINVAL, "PMF_COMPUTE_ERR on CSC data: the reference's frobenius_norm returns its -123456 sentinel there (nmf.py:109-112)");
  if (iters_done) *iters_done = 0;
  if (converged_at) *converged_at = -1;
  if (c->algo == PMF_ALGO_CNMF) {
    PMFCHK(cnmf_ready(c));
    CnmfLoopSteps s{cw, ch, niter};
    return factorize_loop(c, s, niter, ce, conv_eps, ferr, iters_done, converged_at);
  }
  if (!a.nmf_family) {           // W step, then H step, iteration by iteration
    // (a family that takes dense data in both steps refuses whichever of them are on)
    if (c->v_csr && a.dense_w && a.dense_h) return fail(c, PMF_EINVAL, std::string(a.family) + ": dense data only");
    TableLoopSteps s{a, cw, ch};
    return factorize_loop(c, s, niter, ce, conv_eps, ferr, iters_done, converged_at);
  }
  WPipeGuard wguard{c};
  NmfLoopSteps s = nmf_loop_steps(c, niter, cw, ch, ce);
  PMFCHK(factorize_loop(c, s, niter, ce, conv_eps, ferr, iters_done, converged_at));
  wguard.ok = true;              // (the loop's close joined the side stream)
  PMFCHK(ipc_check(c));
  return check_singular(c);
}

int pmf_cluster_get_assigned(pmf_ctx* c, int32_t* assigned) {
  if (!c || !assigned) return fail(c, PMF_EINVAL, "pmf_cluster_get_assigned: bad arguments");
  if (c->algo != PMF_ALGO_KMEANS) return fail(c, PMF_EINVAL, "pmf_cluster_get_assigned: Kmeans only");
  if (!c->cl_have_asg) return fail(c, PMF_EINVAL, "pmf_cluster_get_assigned: no assignment yet (update_h has not run)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(assigned, c->dClAsg, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

int pmf_sivm_get_select(pmf_ctx* c, int32_t* select) {
  if (!c || !select) return fail(c, PMF_EINVAL, "pmf_sivm_get_select: bad arguments");
  if (c->algo != PMF_ALGO_SIVM && c->algo != PMF_ALGO_GREEDY) return fail(c, PMF_EINVAL, "pmf_sivm_get_select: SIVM and GREEDY only");
  if (!c->sv_have_select) return fail(c, PMF_EINVAL, "pmf_sivm_get_select: no selection yet (update_w has not run)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(select, c->dSvSel, (size_t)c->k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

int pmf_sivm_get_volumes(pmf_ctx* c, double* volumes) {
  if (!c || !volumes) return fail(c, PMF_EINVAL, "pmf_sivm_get_volumes: bad arguments");
  if (c->algo != PMF_ALGO_SIVM || !c->sv_sgreedy) return fail(c, PMF_EINVAL, "pmf_sivm_get_volumes: SIVM contexts under sivm_sgreedy only");
  if (!c->sv_have_select || !c->sg_have_vol) return fail(c, PMF_EINVAL, "pmf_sivm_get_volumes: no selection yet (update_w has not run)");
  HIPCHK(c, hipSetDevice(c->device));
  return sgreedy_get_volumes(c, volumes);
}

int pmf_gsat_start(pmf_ctx* c, const int32_t* select, int32_t force, int32_t* started) {
  if (!c || !select) return fail(c, PMF_EINVAL, "pmf_gsat_start: bad arguments");
  PMFCHK(gsat_usable(c, "pmf_gsat_start"));
  PMFCHK(need(c, true, true, false));
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_gsat_start: one rank only in this build");
  if (started) *started = 0;
  if (c->gs_started && !force) return PMF_OK;
  PMFCHK(gsat_start(c, select));
  if (started) *started = 1;
  return PMF_OK;
}

int pmf_gsat_walk(pmf_ctx* c, const int64_t* idx, int64_t n, int32_t* slots_out) {
  if (!c || (n > 0 && (!idx || !slots_out))) return fail(c, PMF_EINVAL, "pmf_gsat_walk: bad arguments");
  PMFCHK(gsat_usable(c, "pmf_gsat_walk"));
  PMFCHK(need(c, true, true, false));
  return gsat_walk(c, idx, n, slots_out);
}

int pmf_gsat_probe_vec(pmf_ctx* c, const float* vec, int32_t* slot_out) {
  if (!c || !vec || !slot_out) return fail(c, PMF_EINVAL, "pmf_gsat_probe_vec: bad arguments");
  PMFCHK(gsat_usable(c, "pmf_gsat_probe_vec"));
  PMFCHK(need(c, true, true, false));
  return gsat_probe_vec(c, vec, slot_out);
}

int pmf_gsat_get_volumes(pmf_ctx* c, double* volumes, int64_t cap, int64_t* count, double* V) {
  if (!c || cap < 0 || (cap > 0 && !volumes)) return fail(c, PMF_EINVAL, "pmf_gsat_get_volumes: bad arguments");
  PMFCHK(gsat_ready(c, "pmf_gsat_get_volumes"));
  if (count) *count = (int64_t)c->gs_log.size();
  if (V) *V = c->gs_V;
  std::copy_n(c->gs_log.begin(), std::min<size_t>((size_t)cap, c->gs_log.size()), volumes);
  return PMF_OK;
}

int pmf_gsat_get_d(pmf_ctx* c, double* D) {
  if (!c || !D) return fail(c, PMF_EINVAL, "pmf_gsat_get_d: bad arguments");
  PMFCHK(need(c, true, true, false));
  return gsat_get_d(c, D);
}

int pmf_greedy_select(pmf_ctx* c, int32_t transposed, int32_t nsel, int32_t* select) {
  if (!c || !select) return fail(c, PMF_EINVAL, "pmf_greedy_select: bad arguments");
  if (c->algo != PMF_ALGO_GREEDY && c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "pmf_greedy_select: GREEDY and CUR / CMD contexts only");
  PMFCHK(cur_csr_refuse(c, "pmf_greedy_select"));
  PMFCHK(need(c, true, false, false));
  return greedy_select_host(c, transposed != 0, nsel, select);
}

int pmf_sivm_select(pmf_ctx* c, int32_t transposed, int32_t nsel, int32_t metric, int32_t init, int32_t path, int32_t* select) {
  if (!c || !select) return fail(c, PMF_EINVAL, "pmf_sivm_select: bad arguments");
  if (c->algo != PMF_ALGO_SIVM && c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "pmf_sivm_select: SIVM and CUR / CMD contexts only");
  PMFCHK(cur_csr_refuse(c, "pmf_sivm_select"));
  PMFCHK(need(c, true, false, false));
  return sivm_select_host(c, transposed != 0, nsel, metric, init, path, select);
}

int pmf_aa_get_beta(pmf_ctx* c, double* beta) {
  if (!c || !beta) return fail(c, PMF_EINVAL, "pmf_aa_get_beta: bad arguments");
  if (c->algo != PMF_ALGO_AA) return fail(c, PMF_EINVAL, "pmf_aa_get_beta: AA only");
  if (!c->aa_have_beta) return fail(c, PMF_EINVAL, "pmf_aa_get_beta: no beta yet (update_w has not run)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(beta, c->dAaBeta, (size_t)c->k * c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

int pmf_aa_rounds(pmf_ctx* c, int32_t* rounds) {
  if (!c || !rounds) return fail(c, PMF_EINVAL, "pmf_aa_rounds: bad arguments");
  if (c->algo != PMF_ALGO_AA) return fail(c, PMF_EINVAL, "pmf_aa_rounds: AA only");
  *rounds = c->aa_rounds;
  return PMF_OK;
}

int pmf_chnmf_hull(pmf_ctx* c, const double* R, int32_t base_sel, int32_t* idx_out, int64_t cap, int64_t* count_out) {
  if (!c || !R || !count_out || cap < 0 || (cap > 0 && !idx_out)) return fail(c, PMF_EINVAL, "pmf_chnmf_hull: bad arguments");
  if (c->algo != PMF_ALGO_AA) return fail(c, PMF_EINVAL, "pmf_chnmf_hull: AA contexts only");
  if (base_sel < 2 || base_sel > PMF_CH_MAX_SEL || base_sel > c->m) return fail(c, PMF_EINVAL, "pmf_chnmf_hull: 2 <= base_sel <= min(16, data_dimension)");
  PMFCHK(need(c, true, false, false));
  if (c->v_csr || !c->dV) return fail(c, PMF_EINVAL, "pmf_chnmf_hull: dense resident data only");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_chnmf_hull: one rank only in this build");
  return chnmf_hull(c, R, base_sel, idx_out, cap, count_out);
}

int pmf_chnmf_set_limits(pmf_ctx* c, int32_t survivor_cap, int32_t max_wgs) {
  if (!c) return PMF_EINVAL;
  if (c->algo != PMF_ALGO_AA) return fail(c, PMF_EINVAL, "pmf_chnmf_set_limits: AA contexts only");
  if (survivor_cap < 0 || survivor_cap > PMF_CH_CAP || max_wgs < 0 || max_wgs > PMF_CL_MAX_WGS)
    return fail(c, PMF_EINVAL, "pmf_chnmf_set_limits: 0 (the build's) <= survivor_cap <= 4096, 0 (the build's) <= max_wgs <= 1024");
  c->ch_cap = survivor_cap; c->ch_max_wgs = max_wgs;
  return PMF_OK;
}

int pmf_chnmf_routes(pmf_ctx* c, int32_t* routes) {
  if (!c || !routes) return fail(c, PMF_EINVAL, "pmf_chnmf_routes: bad arguments");
  if (c->algo != PMF_ALGO_AA) return fail(c, PMF_EINVAL, "pmf_chnmf_routes: AA contexts only");
  for (int r = 0; r < 3; ++r) routes[r] = c->ch_routes[r];
  return PMF_OK;
}

int pmf_vq_columns(pmf_ctx* c, const float* Q, int64_t ldq, int32_t nq, int32_t metric, int32_t* idx_out, double* dist_out) {
  if (!c) return PMF_EINVAL;
  c->hd_synced = false; c->psd_fresh = false;          // (a new API call, as need() notes it; the refusals come before the device is touched)
  PMFCHK(vq_check(c, "pmf_vq_columns", Q, ldq, nq, metric));
  if (!idx_out) return fail(c, PMF_EINVAL, "pmf_vq_columns: idx_out is NULL");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_vq_columns: one rank only in this build");
  HIPCHK(c, hipSetDevice(c->device));
  return vq_columns(c, Q, ldq, nq, metric, idx_out, dist_out);
}

int pmf_vq_assign(pmf_ctx* c, const float* Q, int64_t ldq, int32_t nq, int32_t metric, int32_t* idx_out, double* dist_all) {
  if (!c) return PMF_EINVAL;
  c->hd_synced = false; c->psd_fresh = false;
  PMFCHK(vq_check(c, "pmf_vq_assign", Q, ldq, nq, metric));
  if (!idx_out && !dist_all) return fail(c, PMF_EINVAL, "pmf_vq_assign: idx_out and dist_all are both NULL");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_vq_assign: one rank only in this build");
  HIPCHK(c, hipSetDevice(c->device));
  return vq_assign(c, Q, ldq, nq, metric, idx_out, dist_all);
}

int pmf_svd_decompose(pmf_ctx* c, int32_t* rank) {
  if (c && c->algo != PMF_ALGO_PCA) return fail(c, PMF_EINVAL, "pmf_svd_decompose: PCA / SVD contexts only");
  PMFCHK(need(c, true, false, false));
  PMFCHK(svd_decompose(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (rank) *rank = c->svd_rank;
  return PMF_OK;
}

int pmf_svd_rank(pmf_ctx* c, int32_t* rank) {
  if (!c || !rank) return fail(c, PMF_EINVAL, "pmf_svd_rank: bad arguments");
  if (c->algo != PMF_ALGO_PCA) return fail(c, PMF_EINVAL, "pmf_svd_rank: PCA / SVD contexts only");
  if (!c->svd_valid) return fail(c, PMF_EINVAL, "pmf_svd_rank: no decomposition of the current data (pmf_svd_decompose / pmf_update_w first)");
  *rank = c->svd_rank;
  return PMF_OK;
}

int pmf_svd_get(pmf_ctx* c, double* U, double* S, double* V) {
  if (c && c->algo != PMF_ALGO_PCA) return fail(c, PMF_EINVAL, "pmf_svd_get: PCA / SVD contexts only");
  PMFCHK(need(c, true, false, false));
  return svd_get(c, U, S, V);
}

int pmf_cur_sqnorms(pmf_ctx* c, double* row_sq, double* col_sq) {
  if (c && c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "pmf_cur_sqnorms: CUR / CMD contexts only");
  PMFCHK(need(c, true, false, false));
  return cur_sqnorms(c, row_sq, col_sq);
}

int pmf_cur_leverage(pmf_ctx* c, int32_t k_rows, int32_t k_cols, double* row_lev, double* col_lev) {
  if (c && c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "pmf_cur_leverage: CUR / CMD contexts only");
  PMFCHK(need(c, true, false, false));
  return cur_leverage(c, k_rows, k_cols, row_lev, col_lev);
}

int pmf_cur_compute(pmf_ctx* c, const int32_t* rid, const int32_t* rcnt, int32_t nr, const int32_t* cid, const int32_t* ccnt, int32_t nc) {
  if (c && c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "pmf_cur_compute: CUR / CMD contexts only");
  PMFCHK(need(c, true, false, false));
  return cur_compute(c, rid, rcnt, nr, cid, ccnt, nc);
}

int pmf_cur_get(pmf_ctx* c, double* C, double* U, double* R) {
  if (c && c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "pmf_cur_get: CUR / CMD contexts only");
  PMFCHK(need(c, true, false, false));
  return cur_get(c, C, U, R);
}

int pmf_cur_ferr(pmf_ctx* c, double* out) {
  if (!c || !out) return fail(c, PMF_EINVAL, "pmf_cur_ferr: bad arguments");
  if (c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "pmf_cur_ferr: CUR / CMD contexts only");
  PMFCHK(need(c, true, false, false));
  return cur_ferr(c, out);
}

int pmf_cluster_set_assigned(pmf_ctx* c, const int32_t* assigned) {
  if (!c || !assigned) return fail(c, PMF_EINVAL, "pmf_cluster_set_assigned: bad arguments");
  if (c->algo != PMF_ALGO_KMEANS) return fail(c, PMF_EINVAL, "pmf_cluster_set_assigned: Kmeans only");
  for (int64_t q = 0; q < c->n; ++q)
    if (assigned[q] < 0 || assigned[q] >= c->k) return fail(c, PMF_EINVAL, "pmf_cluster_set_assigned: index out of range");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(c->dClAsg, 0xFF, (size_t)c->np * sizeof(int32_t), c->stream));   // pad columns: -1
  HIPCHK(c, hipMemcpyAsync(c->dClAsg, assigned, (size_t)c->n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->cl_have_asg = true;
  c->cl_sums_valid = false;
  return PMF_OK;
}

int pmf_set_lambda(pmf_ctx* c, double lamb_w, double lamb_h) {
  if (!c) return PMF_EINVAL;
  if (c->algo != PMF_ALGO_BNMF && c->algo != PMF_ALGO_RNMF)
    return fail(c, PMF_EINVAL, "pmf_set_lambda: only BNMF (penalty weights) and RNMF (threshold) take it");
  c->lamb_w = lamb_w; c->lamb_h = lamb_h;
  return PMF_OK;
}

int pmf_get_lambda(pmf_ctx* c, double* lamb_w, double* lamb_h) {
  if (!c || !lamb_w || !lamb_h) return PMF_EINVAL;
  *lamb_w = c->lamb_w; *lamb_h = c->lamb_h;
  return PMF_OK;
}

int pmf_rnmf_update_s(pmf_ctx* c) {
  PMFCHK(need(c, true, true, true));
  if (c->algo != PMF_ALGO_RNMF) return fail(c, PMF_EINVAL, "pmf_rnmf_update_s: RNMF only");
  PMFCHK(rnmf_update_s(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

int pmf_rnmf_get_s_f32(pmf_ctx* c, float* S) {
  PMFCHK(need(c, true, false, false));
  if (c->algo != PMF_ALGO_RNMF || !c->s_valid || !S) return fail(c, PMF_EINVAL, "pmf_rnmf_get_s_f32: no S");
  // S = D + V on the device (the state kept is D = S - data, rnmf.py:102,111), then one download
  DevTemps tmp;
  float* dS = nullptr;
  PMFCHK(talloc(c, tmp, &dS, (size_t)c->mp * c->np));
  const int64_t E = c->mp * c->np;
  hipLaunchKernelGGL(k_add_f32, dim3(elem_grid(E / 4)), dim3(256), 0, c->stream, c->dD, c->dV, E, dS);
  HIPCHK(c, hipGetLastError());
  return download_padded(c, S, c->n, dS, c->np, c->m, c->n);
}

// The reference's S is an attribute: it travels with copies and pickles of the object (the host class hands it to the new
// context here) -- D = S - data, as pmf_rnmf_update_s leaves it.
int pmf_rnmf_set_s_f32(pmf_ctx* c, const float* S) {
  PMFCHK(need(c, true, false, false));
  if (c->algo != PMF_ALGO_RNMF || !S) return fail(c, PMF_EINVAL, "pmf_rnmf_set_s_f32: RNMF only, S must not be NULL");
  if (!c->dD) return fail(c, PMF_EINVAL, "pmf_rnmf_set_s_f32: no device state");
  PMFCHK(upload_padded(c, c->dD, c->np, S, c->n, c->m, c->n));
  c->s_valid = true;
  PMFCHK(rnmf_data_change_end(c));                 // D = S - V
  sums_dropped(c, /*transport=*/false);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

// ---- streamed V: one pass = one reference iteration over row tiles handed in by the caller ------
// (the `data[:, :]` idiom of nmf.py:123,129 for data that does not fit in HBM --
// an h5py dataset, a memmap, a matrix larger than 288 GB.)  W stays resident; a tile is visited once
// per pass: W step on its rows (nmf.py:128-132), then the partials of W^T V and W^T W of the NEW
// rows, accumulated in float64 over the tiles; pmf_stream_end all-reduces them, runs the H step
// (nmf.py:122-126) and evaluates ||V - W H|| by the trace identity.  Copies run on their own
// stream into two device tiles, so the copy of tile t+1 overlaps the kernels of tile t.
int pmf_stream_begin(pmf_ctx* c, uint32_t flags, int64_t max_tile_rows) {
  if (c) c->hd_synced = false;
  if (!c) return PMF_EINVAL;
  PMFCHK(cur_csr_refuse(c, "pmf_stream_*"));
  PMFCHK(svd_csr_refuse(c, "pmf_stream_*"));
  PMFCHK(greedy_csr_refuse(c, "pmf_stream_*"));
  PMFCHK(cluster_csr_refuse(c, "pmf_stream_*"));
  if (!algo_row(c).streamable)
    return fail(c, PMF_EINVAL, "pmf_stream_*: NMF, BNMF, SNMF and NMFALS contexts");
  if (nmf_csr(c)) return fail(c, PMF_EINVAL, "pmf_stream_*: not on an NMF context that holds CSR data (set dense data, or none, first)");
  if (!c->have_w || !c->have_h) return fail(c, PMF_EINVAL, "pmf_stream_begin: W and H must be set");
  if (max_tile_rows < 1) return fail(c, PMF_EINVAL, "pmf_stream_begin: max_tile_rows must be >= 1");
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t cap = std::min<int64_t>(round_up(max_tile_rows, 64), c->mp);
  if (!c->copy_stream) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      HIPCHK(c, hipEventCreateWithFlags(&c->ev_copied[b], hipEventDisableTiming));
      HIPCHK(c, hipEventCreateWithFlags(&c->ev_consumed[b], hipEventDisableTiming));
    }
    PMFCHK(dalloc(c, &c->dPSacc, (size_t)ps_elems(c)));
    PMFCHK(dalloc(c, &c->dStAcc, 4));
  }
  if (cap > c->tile_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    for (int b = 0; b < 2; ++b) {
      PMFCHK(dgrow(c, &c->dTile[b], (size_t)cap * c->np));    // zeroed: pad columns stay 0
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tile_cap = cap;
  }
  c->st_flags = flags;
  c->st_rows_seen = 0;
  c->st_tiles = 0;
  c->st_active = true;
  c->st_vnorm_pending = !(flags & PMF_STREAM_RESID) && !c->vnorm_valid;
  if ((flags & PMF_COMPUTE_W) && !(flags & PMF_STREAM_RESID)) {
    // what the W step of every tile needs from H: G = H H^T (NMF, BNMF); M^T = inv(H H^T) H (SNMF, snmf.py:67-70);
    // the Hessian H H^T in float64 + the warm-start verdict (NMFALS, nmfals.py:85-97)
    if (c->algo == PMF_ALGO_SNMF) PMFCHK(snmf_inverse(c));
    else if (c->algo == PMF_ALGO_NMFALS) { PMFCHK(ensure_gram(c, 1.0)); PMFCHK(nnqp_prepare(c, c->stream, nnqp_use_wave(c))); }
    else PMFCHK(ensure_gram(c, 0.0));
  }
  return PMF_OK;
}

int pmf_stream_tile(pmf_ctx* c, int64_t row0, int64_t rows, const float* tile, int64_t ld) {
  if (!c) return PMF_EINVAL;
  if (!c->st_active) return fail(c, PMF_EINVAL, "pmf_stream_tile: no pass open (pmf_stream_begin)");
  if (!tile || ld < c->n || rows < 1 || rows > c->tile_cap || row0 != c->st_rows_seen || row0 + rows > c->m ||
      (row0 % 64) != 0 || (row0 + rows < c->m && (rows % 64) != 0))
    return fail(c, PMF_EINVAL, "pmf_stream_tile: tiles must arrive in row order, start on a multiple of 64 rows, "
                               "hold a multiple of 64 rows (except the last) and fit max_tile_rows");
  HIPCHK(c, hipSetDevice(c->device));
  const int b = c->st_tiles & 1;
  const int64_t rows_p = round_up(rows, 64);
  float* T = c->dTile[b];
  if (c->st_tiles >= 2) {
    // The copy below is enqueued BEHIND the consumer of this buffer's previous tile and reads the caller's memory when it
    // runs, not now: without a bound the host gets many tiles ahead of the device and a caller that hands over temporaries
    // (a float64 or strided `data` converted tile by tile) frees them long before they are read -- garbage tiles, NaN factors
    // (found by tests/sweeps/fuzz_sequences.py).  Waiting here for the COPY of the tile two calls back bounds the host's lead
    // to the two device tiles: a caller's tile must stay valid until the second-next call (or pmf_stream_end) has returned.
    HIPCHK(c, hipEventSynchronize(c->ev_copied[b]));
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_consumed[b], 0));
  }
  HIPCHK(c, hipMemcpy2DAsync(T, (size_t)c->np * sizeof(float), tile, (size_t)ld * sizeof(float),
                             (size_t)c->n * sizeof(float), (size_t)rows, hipMemcpyHostToDevice, c->copy_stream));
  if (rows_p > rows)
    HIPCHK(c, hipMemsetAsync(T + rows * c->np, 0, (size_t)(rows_p - rows) * c->np * sizeof(float), c->copy_stream));
  HIPCHK(c, hipEventRecord(c->ev_copied[b], c->copy_stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copied[b], 0));
  float* Wt = c->dW + row0 * c->KP;
  const int first = c->st_tiles == 0;
  if (c->st_flags & PMF_STREAM_RESID) {
    if (c->nb > 1) {            // num_bases > 128: launch_resid's kernels end at 128 bases (found by tests/sweeps/fuzz_sequences.py)
      PMFCHK(resid_bigk(c, false, c->dScal + 5, T, Wt, rows_p));
    } else {
      PMFCHK(launch_resid(c, false, 0.f, T, Wt, rows_p));
      hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(256), 0, c->stream, c->dPart, c->resid_parts, c->dScal + 5);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_accum_f64, dim3(1), dim3(64), 0, c->stream, c->dStAcc + 1, c->dScal + 5, first);
    HIPCHK(c, hipGetLastError());
  } else {
    if (c->st_vnorm_pending) {
      const int nb = 256;
      hipLaunchKernelGGL(k_sumsq, dim3(nb), dim3(256), 0, c->stream, T, rows_p * c->np, c->dPart);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(256), 0, c->stream, c->dPart, nb, c->dScal + 5);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(k_accum_f64, dim3(1), dim3(64), 0, c->stream, c->dStAcc, c->dScal + 5, first);
      HIPCHK(c, hipGetLastError());
    }
    if (c->st_flags & PMF_COMPUTE_W) {
      if (c->nb > 1 && (c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_BNMF)) {   // blocks of 128 bases (bigk_update_w)
        PMFCHK(bigk_update_w_rows(c, T, Wt, c->dW1 + row0 * c->KP, c->dW2 + row0 * c->KP, rows_p, rows));
      } else if ((c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_BNMF) && c->np > PMF_WIDE_K) {   // (very wide data)
        PMFCHK(wide_update_w_rows(c, T, Wt, rows_p, rows));
      } else if (c->algo == PMF_ALGO_BNMF) {   // bnmf.py:87-90: the penalised W rule, same contractions
        PMFCHK(rowgemm<EPI_BNMF_W>(c, T, c->np, c->np, c->dH, c->np, Wt, c->dG, nullptr, rows_p, rows));
      } else if (c->algo == PMF_ALGO_SNMF) {   // snmf.py:67-70: the tile's rows of W = V M^T
        PMFCHK(rowgemm<EPI_STORE>(c, T, c->np, c->np, c->dMT, c->np, nullptr, nullptr, Wt, rows_p, rows));
      } else if (c->algo == PMF_ALGO_NMFALS) {  // nmfals.py:85-97: right-hand sides V H^T of the tile's rows, one QP per row
        float* Ft = c->dW1 + row0 * c->KP;
        PMFCHK(rowgemm<EPI_STORE>(c, T, c->np, c->np, c->dH, c->np, nullptr, nullptr, Ft, rows_p, rows));
        if (nnqp_use_wave(c)) {                  // 64 < num_bases <= 128: k_nnqp_wave, inv(HA) prepared by pmf_stream_begin
          PMFCHK(solve_nnqps(c, Ft, 1, c->KP, Wt, 1, c->KP, rows, false, true));
        } else {
          double* qp = nullptr;
          PMFCHK(nnqp_scratch(c, &qp));
          const int qrc = pmf_launch_nnqp(c->stream, c->KP, c->k, c->dGd, Ft, 1, c->KP, Wt, 1, c->KP, rows, c->dWarm, qp, 0);
          if (qrc != PMF_OK) return fail(c, qrc, "nnqp launch (streamed W tile) failed");
          HIPCHK(c, hipGetLastError());
        }
      } else {
        PMFCHK(rowgemm<EPI_NMF_W>(c, T, c->np, c->np, c->dH, c->np, Wt, c->dG, nullptr, rows_p, rows));
      }
      c->ps_valid = false; c->num_valid = false; c->trace_ready = false;
    }
    if ((c->st_flags & (PMF_COMPUTE_H | PMF_COMPUTE_ERR)) && !((c->st_flags & PMF_COMPUTE_W) == 0 && c->ps_valid)) {
      const int64_t blocks16 = rows_p / 16;
      int tch = (int)std::min<int64_t>(c->nchunks, blocks16);
      const int rpc = (int)round_up((blocks16 + tch - 1) / tch, 4) * 16;
      tch = (int)((rows_p + rpc - 1) / rpc);
      if (c->nb > 1) {
        PMFCHK(bigk_ps_rows(c, T, Wt, rows_p, rpc, tch, c->dPSacc, first));
      } else {
      PMFCHK(colgemm_rows(c, T, Wt, rows_p, rpc, tch));
      const int64_t E = ps_elems(c);
      hipLaunchKernelGGL(k_reduce_slabs_acc, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, c->stream, c->dSlab, tch,
                         E, c->dPSacc, first);
      HIPCHK(c, hipGetLastError());
      }
    }
  }
  HIPCHK(c, hipEventRecord(c->ev_consumed[b], c->stream));
  c->st_rows_seen += rows;
  c->st_tiles += 1;
  return PMF_OK;
}

int pmf_stream_end(pmf_ctx* c, double* ferr, int32_t* needs_direct) {
  if (!c) return PMF_EINVAL;
  if (!c->st_active) return fail(c, PMF_EINVAL, "pmf_stream_end: no pass open");
  c->st_active = false;
  c->hd_synced = false;
  if (needs_direct) *needs_direct = 0;
  if (c->st_rows_seen != c->m)
    return fail(c, PMF_EINVAL, "pmf_stream_end: the tiles covered " + std::to_string(c->st_rows_seen) + " of " +
                std::to_string(c->m) + " rows");
  HIPCHK(c, hipSetDevice(c->device));
  if (c->st_flags & PMF_STREAM_RESID) {
    PMFCHK(allreduce_sum(c, c->dStAcc + 1, 1, true));
    double ss = 0.0;
    HIPCHK(c, hipMemcpyAsync(&ss, c->dStAcc + 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ferr) *ferr = std::sqrt(ss);
    return PMF_OK;
  }
  if (c->st_vnorm_pending) {
    PMFCHK(allreduce_sum(c, c->dStAcc, 1, true));
    HIPCHK(c, hipMemcpyAsync(&c->vnorm2, c->dStAcc, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->vnorm_valid = true;
    c->st_vnorm_pending = false;
  }
  const bool need_ps = (c->st_flags & (PMF_COMPUTE_H | PMF_COMPUTE_ERR)) != 0;
  if (need_ps && !c->ps_valid) {
    const int64_t E = ps_elems(c);
    hipLaunchKernelGGL(k_f64_to_f32, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, c->stream, c->dPSacc, E, c->dPS);
    HIPCHK(c, hipGetLastError());
    PMFCHK(allreduce_ps(c));
    c->ps_valid = true;
    c->trace_ready = false;       // (terms an earlier H step left belong to an earlier (P | S))
  }
  if (c->st_flags & PMF_COMPUTE_H) {
    c->want_trace = (c->st_flags & PMF_COMPUTE_ERR) != 0;
    const int rc = c->algo == PMF_ALGO_NMFALS ? als_update_h(c) : h_step_from_ps(c);   // nmfals.py:70-82: QPs over the summed (P | S)
    c->want_trace = false;
    PMFCHK(rc);
  }
  if ((c->st_flags & PMF_COMPUTE_ERR) && ferr) {
    double e2 = 0.0;
    PMFCHK(trace_e2(c, &e2));
    if (!(e2 > 1e-3 * c->vnorm2) && needs_direct) *needs_direct = 1;   // cancellation: ask for a PMF_STREAM_RESID pass
    *ferr = std::sqrt(e2 > 0.0 ? e2 : 0.0);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return check_singular(c);
}

int pmf_nndsvd_init(pmf_ctx* c, int32_t* rank_found) {
  PMFCHK(need(c, true, false, false));
  if (c->algo == PMF_ALGO_RNMF || c->algo == PMF_ALGO_CNMF) return fail(c, PMF_EINVAL, "pmf_nndsvd_init: not for RNMF / CNMF contexts");
  PMFCHK(svd_csr_refuse(c, "pmf_nndsvd_init"));
  PMFCHK(greedy_csr_refuse(c, "pmf_nndsvd_init"));
  PMFCHK(cluster_csr_refuse(c, "pmf_nndsvd_init"));
  return nndsvd_init(c, rank_found);
}

int pmf_cnmf_init(pmf_ctx* c, const int32_t* sel, int32_t km_niter, int32_t* assigned_out) {
  PMFCHK(need(c, true, false, false));
  if (c->algo != PMF_ALGO_CNMF) return fail(c, PMF_EINVAL, "pmf_cnmf_init: CNMF contexts only");
  if (c->v_csr) return fail(c, PMF_EINVAL, "CNMF: dense data only");
  if (!sel || km_niter < 0) return fail(c, PMF_EINVAL, "pmf_cnmf_init: bad arguments");
  for (int j = 0; j < c->k; ++j)
    if (sel[j] < 0 || sel[j] >= c->n || (j > 0 && sel[j] <= sel[j - 1]))
      return fail(c, PMF_EINVAL, "pmf_cnmf_init: sel must be num_bases sorted distinct sample indices");
  PMFCHK(cnmf_alloc(c));
  PMFCHK(cnmf_ensure_c(c));
  PMFCHK(dgrow(c, &c->dFerr, &c->ferr_cap, (int64_t)km_niter + 1));
  // Kmeans(data, num_bases).factorize(niter=km_niter) (cnmf.py:84-86): init_w = the selected samples, init_h = one assignment,
  // then update_w, update_h and the error per iteration with the reference's early exit -- no host round trip in between
  HIPCHK(c, hipMemcpyAsync(c->dKmSel, sel, (size_t)c->k * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->dStop, 0, 2 * sizeof(int), c->stream));
  const int64_t E = (int64_t)c->KP * c->np;
  const dim3 egrid((unsigned)std::min<int64_t>((E + 255) / 256, 2048));
  hipLaunchKernelGGL(k_kmeans_seed, egrid, dim3(256), 0, c->stream, c->dCnHn, c->np, c->KP, c->k, (const int*)c->dKmSel);
  HIPCHK(c, hipGetLastError());
  PMFCHK(kmeans_assign_pass(c, -1, 1e-8));
  for (int it = 0; it < km_niter; ++it) {
    hipLaunchKernelGGL(k_kmeans_update, egrid, dim3(256), 0, c->stream, c->dCnHn, (int)c->n, c->np, c->k, (const int*)c->dKmAsg,
                       (const int*)c->dKmCnt, (const int*)c->dStop);
    HIPCHK(c, hipGetLastError());
    PMFCHK(kmeans_assign_pass(c, it, 1e-8));                 // nmf.py:69 (_EPS), kmeans.py:76-81
  }
  // CNMF.init_h (cnmf.py:88-100): H from the assignment; G too unless the caller has set one
  const bool with_g = !c->have_g;
  hipLaunchKernelGGL(k_cnmf_init_hg, egrid, dim3(256), 0, c->stream, (const int*)c->dKmAsg, (const int*)c->dKmCnt, (int)c->n, c->np,
                     c->KP, c->k, c->dHd, c->dH, c->dGT, 1, with_g ? 1 : 0);
  HIPCHK(c, hipGetLastError());
  if (assigned_out)
    HIPCHK(c, hipMemcpyAsync(assigned_out, c->dKmAsg, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  h_replaced(c, true, false);        // (Hd and its rounding H written together)
  if (with_g) g_replaced(c);
  return PMF_OK;
}

int pmf_set_g_f64(pmf_ctx* c, const double* G) {
  if (!c || !G) return fail(c, PMF_EINVAL, "pmf_set_g_f64: bad arguments");
  if (c->algo != PMF_ALGO_CNMF) return fail(c, PMF_EINVAL, "pmf_set_g_f64: CNMF contexts only");
  HIPCHK(c, hipSetDevice(c->device));
  PMFCHK(cnmf_alloc(c));
  const size_t bytes = (size_t)c->n * c->k * sizeof(double);
  PMFCHK(stage_reserve(c, bytes));
  HIPCHK(c, hipMemcpyAsync(c->dStage, G, bytes, hipMemcpyHostToDevice, c->stream));
  const int64_t E = (int64_t)c->KP * c->np;
  hipLaunchKernelGGL(k_cnmf_g_to_gt, dim3((unsigned)std::min<int64_t>((E + 255) / 256, 2048)), dim3(256), 0, c->stream,
                     reinterpret_cast<const double*>(c->dStage), (int)c->n, c->k, c->np, c->KP, c->dGT);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->cn_user_w) PMFCHK(w_pipe_join(c));     // (W = V G of the new G from here on)
  g_replaced(c);
  return PMF_OK;
}

int pmf_get_g_f64(pmf_ctx* c, double* G) {
  PMFCHK(need(c, false, false, false));
  if (!G) return fail(c, PMF_EINVAL, "G is NULL");
  if (c->algo != PMF_ALGO_CNMF) return fail(c, PMF_EINVAL, "pmf_get_g_f64: CNMF contexts only");
  if (!c->have_g) return fail(c, PMF_EINVAL, "G has not been set (pmf_set_g_f64 / pmf_cnmf_init)");
  const size_t bytes = (size_t)c->n * c->k * sizeof(double);
  PMFCHK(stage_reserve(c, bytes));
  const int64_t E = (int64_t)c->n * c->k;
  hipLaunchKernelGGL(k_cnmf_gt_to_g, dim3((unsigned)std::min<int64_t>((E + 255) / 256, 2048)), dim3(256), 0, c->stream, c->dGT, (int)c->n,
                     c->k, c->np, reinterpret_cast<double*>(c->dStage));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(G, c->dStage, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}


int pmf_nnqp_counters(pmf_ctx* c, int64_t* out8, int32_t reset) {
  if (!c || !out8) return PMF_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c->dQstat) {
    HIPCHK(c, hipMemcpyAsync(h, c->dQstat, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    if (reset) HIPCHK(c, hipMemsetAsync(c->dQstat, 0, sizeof(h), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  for (int q = 0; q < 8; ++q) out8[q] = (int64_t)h[q];
  return PMF_OK;
}

int pmf_last_loop_ms(pmf_ctx* c, double* ms) {
  if (!c || !ms) return PMF_EINVAL;
  *ms = c->last_loop_ms;
  return PMF_OK;
}

int pmf_collective_ms(pmf_ctx* c, double* mean_ms, int64_t* count) {
  if (!c || !mean_ms || !count) return PMF_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double sum = 0.0;
  int64_t n = 0;
  for (size_t q = 0; q + 1 < c->coll_used; q += 2) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->coll_ev[q], c->coll_ev[q + 1]) == hipSuccess) { sum += ms; ++n; }
  }
  if (c->dIpcWait) {
    // the folded exchanges have no launch to bracket: what they cost an iteration is the consumer's wait for the slowest
    // peer's flags in k_nmf_h_gram's prologue (ticks of the 100 MHz counter, summed on the device since pmf_profile_enable)
    unsigned long long w[2] = {0, 0};
    HIPCHK(c, hipMemcpy(w, c->dIpcWait, sizeof(w), hipMemcpyDeviceToHost));
    sum += (double)w[0] * 1e-5;        // 100 MHz ticks -> ms
    n += (int64_t)w[1];
  }
  *mean_ms = n ? sum / (double)n : 0.0;
  *count = n;
  return PMF_OK;
}

int pmf_profile_enable(pmf_ctx* c, int32_t on) {
  if (!c) return PMF_EINVAL;
  c->profile = on != 0;
  c->stat.used = 0;
  c->stat.seen = 0;
  c->stat.open = false;
  c->coll_seen = 0;
  c->coll_used = 0;
  if (c->dIpcWait) HIPCHK(c, hipMemsetAsync(c->dIpcWait, 0, 2 * sizeof(unsigned long long), c->stream));
  return PMF_OK;
}

int pmf_kernel_stats(pmf_ctx* c, const char** name, int64_t* launches, double* mean_ms,
                     double* flops_per_launch, double* bytes_per_launch) {
  if (!c) return PMF_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double tot = 0.0;
  const size_t pairs = c->stat.used / 2;
  for (size_t q = 0; q < pairs; ++q) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->stat.ev[2 * q], c->stat.ev[2 * q + 1]));
    tot += ms;
  }
  if (name) *name = c->stat.name.c_str();
  if (launches) *launches = (int64_t)pairs;
  if (mean_ms) *mean_ms = pairs ? tot / (double)pairs : 0.0;
  if (flops_per_launch) *flops_per_launch = c->stat.flops;
  if (bytes_per_launch) *bytes_per_launch = c->stat.bytes;
  return PMF_OK;
}

// ---- host-side change detector for the caller's arrays (no device involved) -------------------
// The reference computes from whatever self.W / self.H / self.data hold at the time of the call
// (nmf.py:122-132); the host class keeps device copies and must notice ANY in-place edit of the host
// arrays.  A sum misses permutations; this is an order-dependent 128-bit digest of the raw bytes:
// 8 interleaved multiply-rotate lanes per 64-byte line (memory speed), 8 MiB chunks hashed by up to
// 16 threads and folded in chunk order.
static inline uint64_t pmf_rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
static inline uint64_t pmf_fmix64(uint64_t h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h;
}
static void pmf_hash_chunk(const unsigned char* p, size_t n, uint64_t seed, uint64_t out[2]) {
  constexpr uint64_t P1 = 0x9e3779b185ebca87ull, P2 = 0xc2b2ae3d27d4eb4full;
  uint64_t a[8];
  for (int l = 0; l < 8; ++l) a[l] = pmf_fmix64(seed + P1 * (uint64_t)(l + 1));
  const size_t lines = n / 64;
  for (size_t i = 0; i < lines; ++i) {
    uint64_t w[8];
    std::memcpy(w, p + 64 * i, 64);
    for (int l = 0; l < 8; ++l) a[l] = (pmf_rotl64(a[l], 31) ^ w[l]) * P1;
  }
  if (n % 64) {
    uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::memcpy(w, p + 64 * lines, n % 64);
    for (int l = 0; l < 8; ++l) a[l] = (pmf_rotl64(a[l], 31) ^ w[l]) * P1;
  }
  uint64_t h1 = (uint64_t)n * P2, h2 = seed ^ P2;
  for (int l = 0; l < 8; ++l) {
    h1 = pmf_rotl64(h1, 27) * P1 + pmf_fmix64(a[l]);
    h2 = (pmf_rotl64(h2, 29) ^ pmf_fmix64(a[l] + P2 * (uint64_t)(l + 1))) * P2;
  }
  out[0] = pmf_fmix64(h1);
  out[1] = pmf_fmix64(h2);
}

int pmf_host_checksum(const void* data, uint64_t nbytes, uint64_t* out2) {
  if (!out2 || (nbytes && !data)) return PMF_EINVAL;
  const unsigned char* p = static_cast<const unsigned char*>(data);
  constexpr size_t CH = (size_t)8 << 20;
  const size_t nch = nbytes ? (size_t)((nbytes + CH - 1) / CH) : 1;
  std::vector<uint64_t> dig(2 * nch);
  auto work = [&](size_t c0, size_t c1) {
    for (size_t q = c0; q < c1; ++q) {
      const size_t off = q * CH;
      pmf_hash_chunk(p + off, (size_t)std::min<uint64_t>(CH, nbytes - off), 0x243f6a8885a308d3ull + q, &dig[2 * q]);
    }
  };
  unsigned nthr = std::min<unsigned>(std::min<size_t>(nch, 16), std::max(1u, std::thread::hardware_concurrency()));
  if (nthr <= 1) {
    work(0, nch);
  } else {
    std::vector<std::thread> th;
    bool spawned_all = true;
    size_t next = 0;
    try {
      for (unsigned t = 0; t < nthr; ++t) {
        const size_t c0 = nch * t / nthr, c1 = nch * (t + 1) / nthr;
        th.emplace_back(work, c0, c1);
        next = c1;
      }
    } catch (...) { spawned_all = false; }
    for (auto& t : th) t.join();
    if (!spawned_all) work(next, nch);
  }
  uint64_t h1 = 0x13198a2e03707344ull ^ nbytes, h2 = 0xa4093822299f31d0ull;
  for (size_t q = 0; q < nch; ++q) {
    h1 = pmf_fmix64(pmf_rotl64(h1, 23) * 0x9e3779b185ebca87ull + dig[2 * q]);
    h2 = pmf_fmix64((pmf_rotl64(h2, 37) ^ dig[2 * q + 1]) * 0xc2b2ae3d27d4eb4full);
  }
  out2[0] = h1;
  out2[1] = h2;
  return PMF_OK;
}

int pmf_set_option(pmf_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return PMF_EINVAL;
  if (std::strcmp(name, "force_tiled") == 0) {
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "force_tiled: 0 or 1");
    if (value == 1 && c->fused_wgs > 0) {
      c->fused_wgs_hidden = c->fused_wgs; c->fused8_hidden = c->fused8;
      c->fused_wgs = 0; c->fused8 = false;
      c->path_hidden = c->path;
      c->path = "tiled (forced)";
    } else if (value == 0 && c->fused_wgs_hidden > 0) {
      c->fused_wgs = c->fused_wgs_hidden; c->fused8 = c->fused8_hidden;
      c->fused_wgs_hidden = 0;
      c->path = c->path_hidden;
    }
    c->ps_valid = false; c->num_valid = false; c->trace_ready = false;
    if (c->g_parts > 0) { c->g_valid = false; c->g_parts = 0; }
    choose_stat_site(c, false);
    return PMF_OK;
  }
  if (std::strcmp(name, "profile_every") == 0) {
    if (value < 1 || value > 1 << 20) return fail(c, PMF_EINVAL, "profile_every: 1 .. 2^20");
    c->stat.every = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "fold_exchange") == 0) {
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "fold_exchange: 0 or 1");
    c->opt_fold = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "oneshot_allreduce") == 0) {
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "oneshot_allreduce: 0 or 1");
    if (value == 1 && c->ipc_nranks_ready <= 1) return fail(c, PMF_EINVAL, "oneshot_allreduce: not set up (pmf_ipc_export / pmf_ipc_import)");
    c->ipc.nranks = value ? c->ipc_nranks_ready : 0;
    return PMF_OK;
  }
  if (std::strcmp(name, "nnqp_wave") == 0) {
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "nnqp_wave: 0 or 1");
    c->opt_nnqp_wave = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "snmf_w_pipe") == 0) {
    if (value < 0 || value > 256) return fail(c, PMF_EINVAL, "snmf_w_pipe: 0 (off) .. 256 workgroup slots left free by the W write");
    HIPCHK(c, hipSetDevice(c->device));
    PMFCHK(w_pipe_join(c));
    c->opt_w_pipe = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "nnqp_count") == 0) {
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "nnqp_count: 0 or 1");
    c->opt_nnqp_count = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "nnqp_frame16") == 0) {
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "nnqp_frame16: 0 or 1");
    c->opt_nnqp_frame16 = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "nnqp_quad") == 0) {
    if (value < 0 || value > 2) return fail(c, PMF_EINVAL, "nnqp_quad: 0 (never), 1 (from 16 384 problems per half step on) or 2 (always)");
    c->opt_nnqp_quad = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "nndsvd_topk") == 0) {
    if (value < -1 || value > 1) return fail(c, PMF_EINVAL, "nndsvd_topk: -1 (by size), 0 or 1");
    c->opt_nndsvd_topk = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "colgemm_stream") == 0) {
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "colgemm_stream: 0 or 1");
    c->opt_colgemm_stream = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "rowgemm_stream") == 0) {
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "rowgemm_stream: 0 or 1");
    c->opt_rowgemm_stream = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "svd_num_triples") == 0) {
    if (c->algo != PMF_ALGO_PCA) return fail(c, PMF_EINVAL, "svd_num_triples: PCA / SVD contexts only");
    if (value < 0 || value > PMF_GRAM_MAX_NP) return fail(c, PMF_EINVAL, "svd_num_triples: 0 (all) .. 1024");
    if (c->svd_triples != (int)value && c->v_csr) c->svd_valid = false;     // (a decomposition of CSR data kept another count)
    c->svd_triples = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "pca_num_bases") == 0) {
    if (c->algo != PMF_ALGO_PCA) return fail(c, PMF_EINVAL, "pca_num_bases: PCA / SVD contexts only");
    if (value < 0 || value > c->k) return fail(c, PMF_EINVAL, "pca_num_bases: 0 (all) .. the context's base count");
    c->pca_bases = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "sivm_metric") == 0 || std::strcmp(name, "sivm_init") == 0) {
    if (c->algo != PMF_ALGO_SIVM) return fail(c, PMF_EINVAL, "sivm_metric / sivm_init: SIVM contexts only");
    if (name[5] == 'm') {
      if (value < 0 || value > 2) return fail(c, PMF_EINVAL, "sivm_metric: 0 (l2), 1 (l1) or 2 (cosine)");
      c->sv_metric = (int)value;
      choose_stat_site(c, false);
    } else {
      if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "sivm_init: 0 (fastmap) or 1 (origin)");
      c->sv_init = (int)value;
    }
    return PMF_OK;
  }
  if (std::strcmp(name, "sivm_rule") == 0 || std::strcmp(name, "gmap_method") == 0) {
    if (c->algo != PMF_ALGO_SIVM) return fail(c, PMF_EINVAL, "sivm_rule / gmap_method: SIVM contexts only");
    if (name[0] == 's') {
      if (value < 0 || value > 2) return fail(c, PMF_EINVAL, "sivm_rule: 0 (SIVM), 1 (LAESA) or 2 (GMAP)");
      if (value != 0 && c->sv_sgreedy) return fail(c, PMF_EINVAL, "sivm_rule: LAESA and GMAP not together with sivm_sgreedy");
      if (value != 0 && c->sv_gsat) return fail(c, PMF_EINVAL, "sivm_rule: LAESA and GMAP not together with sivm_gsat");
      c->sv_rule = (int)value;
    } else {
      if (value < 0 || value > 2) return fail(c, PMF_EINVAL, "gmap_method: 0 (pca), 1 (aa) or 2 (nmf)");
      c->sv_gmap_method = (int)value;
    }
    choose_stat_site(c, false);
    return PMF_OK;
  }
  if (std::strcmp(name, "sivm_csc_team") == 0) {
    if (c->algo != PMF_ALGO_SIVM) return fail(c, PMF_EINVAL, "sivm_csc_team: SIVM contexts only");
    if (value != 0 && value != 4 && value != 16 && value != 64) return fail(c, PMF_EINVAL, "sivm_csc_team: 0 (by the mean column length), 4, 16 or 64");
    c->opt_sivm_csc_team = (int)value;
    if (c->v_csc) sivm_csc_name_path(c);
    return PMF_OK;
  }
  if (std::strcmp(name, "sivm_sgreedy") == 0) {
    if (c->algo != PMF_ALGO_SIVM) return fail(c, PMF_EINVAL, "sivm_sgreedy: SIVM contexts only");
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "sivm_sgreedy: 0 or 1");
    if (value == 1 && c->sv_rule != 0) return fail(c, PMF_EINVAL, "sivm_sgreedy: not together with sivm_rule 1 (LAESA) or 2 (GMAP)");
    if (value == 1 && c->sv_gsat) return fail(c, PMF_EINVAL, "sivm_sgreedy: not together with sivm_gsat");
    if ((int)value != c->sv_sgreedy) c->sg_have_vol = false;
    c->sv_sgreedy = (int)value;
    choose_stat_site(c, false);
    return PMF_OK;
  }
  if (std::strcmp(name, "sivm_gsat") == 0) {
    if (c->algo != PMF_ALGO_SIVM) return fail(c, PMF_EINVAL, "sivm_gsat: SIVM contexts only");
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "sivm_gsat: 0 or 1");
    if (value == 1 && (c->sv_rule != 0 || c->sv_sgreedy)) return fail(c, PMF_EINVAL, "sivm_gsat: not together with sivm_rule 1 (LAESA) or 2 (GMAP) or sivm_sgreedy");
    if ((int)value != c->sv_gsat) c->gs_started = false;
    c->sv_gsat = (int)value;
    return PMF_OK;
  }
  if (std::strcmp(name, "profile_sivm_rows") == 0) {
    if (c->algo != PMF_ALGO_SIVM && c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "profile_sivm_rows: SIVM and CUR / CMD contexts only");
    if (value != 0 && value != 1) return fail(c, PMF_EINVAL, "profile_sivm_rows: 0 or 1");
    c->opt_profile_sivm_rows = (int)value;
    choose_stat_site(c, false);
    return PMF_OK;
  }
  if (std::strcmp(name, "profile_cur") == 0) {
    if (c->algo != PMF_ALGO_CUR) return fail(c, PMF_EINVAL, "profile_cur: CUR / CMD contexts only");
    if (value < 0 || value > 2) return fail(c, PMF_EINVAL, "profile_cur: 0 (the cross product), 1 (k_lev_f64) or 2 (k_cur_sqnorms)");
    c->opt_profile_cur = (int)value;
    choose_stat_site(c, false);
    return PMF_OK;
  }
  if (std::strcmp(name, "profile_vq") == 0) {
    if (value < 0 || value > 2) return fail(c, PMF_EINVAL, "profile_vq: 0 (the context's own kernel), 1 (k_vq_pass) or 2 (k_vq_argmin_rows)");
    c->opt_profile_vq = (int)value;
    choose_stat_site(c, false);
    return PMF_OK;
  }
  if (std::strcmp(name, "profile_gather") == 0) {
    if (value < 0 || value > 1) return fail(c, PMF_EINVAL, "profile_gather: 0 (the context's own kernel) or 1 (k_gather_cols)");
    c->opt_profile_gather = (int)value;
    choose_stat_site(c, false);
    return PMF_OK;
  }
  if (std::strcmp(name, "snmf_gram") == 0) {
    if (value < -1 || value > 2) return fail(c, PMF_EINVAL, "snmf_gram: -1 (auto), 0 (off), 1 (on) or 2 (on, W written every iteration)");
    c->opt_snmf_gram = (int)value;
    return PMF_OK;
  }
  return fail(c, PMF_EINVAL, std::string("pmf_set_option: unknown option '") + name + "'");
}

int pmf_set_host_allreduce(pmf_ctx* c, pmf_host_allreduce_fn fn, void* user) {
  if (!c) return PMF_EINVAL;
  if (fn && c->comm) return fail(c, PMF_EINVAL, "pmf_set_host_allreduce: the context already has an RCCL communicator");
  c->host_ar = fn;
  c->host_ar_user = user;
  sums_dropped(c, /*transport=*/true);
  return PMF_OK;
}

// ---- one-shot all-reduce over IPC-mapped receive areas (pmf_ipc.h) ----
int pmf_ipc_export(pmf_ctx* c, int32_t rank, int32_t nranks, void* handle_out) {
  static_assert(sizeof(hipIpcMemHandle_t) <= PMF_IPC_HANDLE_BYTES, "hipIpcMemHandle_t size");
  if (!c || !handle_out || nranks < 2 || nranks > PMF_IPC_MAX_RANKS || rank < 0 || rank >= nranks)
    return fail(c, PMF_EINVAL, "pmf_ipc_export: 2 <= nranks <= 8, 0 <= rank < nranks");
  if (c->ipc_exported) return fail(c, PMF_EINVAL, "pmf_ipc_export: already exported");
  HIPCHK(c, hipSetDevice(c->device));
  void* area = nullptr;
  const size_t bytes = pmf_ipc_area_bytes(nranks);
  // fine-grained device memory: stores of a peer on another GPU must become visible WHILE this rank's kernel polls
  hipError_t e = hipExtMallocWithFlags(&area, bytes, hipDeviceMallocFinegrained);
  hipIpcMemHandle_t h;
  if (e == hipSuccess && hipIpcGetMemHandle(&h, area) != hipSuccess) { (void)hipFree(area); area = nullptr; e = hipErrorUnknown; }
  if (e != hipSuccess) {                       // (a runtime that cannot export fine-grained memory: ordinary device memory)
    (void)hipGetLastError();
    // ... which is only sound between processes on ONE device: coarse-grained memory is, by the memory model, touched by a single
    // agent while a kernel runs -- a peer GPU's stores would meet stale L2 lines here.  With an RCCL communicator (ranks on GPUs of
    // their own) the export fails instead and RCCL keeps carrying the sums.
    if (c->comm != nullptr)
      return fail(c, PMF_EHIP, "pmf_ipc_export: fine-grained device memory cannot be allocated / exported on this runtime");
    HIPCHK(c, hipMalloc(&area, bytes));
    HIPCHK(c, hipIpcGetMemHandle(&h, area));
  }
  HIPCHK(c, hipMemsetAsync(area, 0, bytes, c->stream));
  if (!c->dIpcErr) PMFCHK(dalloc(c, &c->dIpcErr, 1));
  if (!c->dIpcWait) {
    PMFCHK(dalloc(c, &c->dIpcWait, 2));
  }
  // the self-test's two payload buffers, here: everything that can fail on ONE rank alone happens before the ranks vote on
  // "exported"; between the self-test's collectives nothing is allocated
  for (float** p : {&c->dIpcTestA, &c->dIpcTestB}) if (!*p) PMFCHK(dalloc_raw(c, p, PMF_IPC_MAX_BYTES / sizeof(float)));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memset(handle_out, 0, PMF_IPC_HANDLE_BYTES);
  std::memcpy(handle_out, &h, sizeof(h));
  c->ipc = IpcPeers{};
  c->ipc.area[rank] = static_cast<char*>(area);
  c->ipc.me = rank;
  c->ipc.nranks = 0;                          // ready only after pmf_ipc_import
  c->ipc_exported = true;
  c->ipc_export_nranks = nranks;              // the receive area is sized for THIS many ranks
  c->ipc_seq = 0;
  return PMF_OK;
}

int pmf_ipc_import(pmf_ctx* c, const void* handles, int32_t nranks) {
  if (!c || !handles || !c->ipc_exported || nranks != c->ipc_export_nranks || c->ipc_nranks_ready > 0)
    return fail(c, PMF_EINVAL, "pmf_ipc_import: call pmf_ipc_export first, once; handles = nranks x PMF_IPC_HANDLE_BYTES in rank "
                               "order with the nranks given to pmf_ipc_export (the receive areas are sized for it)");
  HIPCHK(c, hipSetDevice(c->device));
  for (int r = 0; r < nranks; ++r) {
    if (r == c->ipc.me) continue;
    hipIpcMemHandle_t h;
    std::memcpy(&h, static_cast<const char*>(handles) + (size_t)r * PMF_IPC_HANDLE_BYTES, sizeof(h));
    void* p = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {                     // give back what was mapped so far: nothing half-open survives a failed import
      (void)hipGetLastError();
      for (int q = 0; q < nranks; ++q)
        if (q != c->ipc.me && c->ipc.area[q]) { (void)hipIpcCloseMemHandle(c->ipc.area[q]); c->ipc.area[q] = nullptr; }
      return fail(c, PMF_EHIP, std::string("pmf_ipc_import: hipIpcOpenMemHandle of rank ") + std::to_string(r) + ": " + hipGetErrorString(e));
    }
    c->ipc.area[r] = static_cast<char*>(p);
  }
  c->ipc.nranks = nranks;
  c->ipc_nranks_ready = nranks;
  return PMF_OK;
}

// The one-shot path against the context's other transport (RCCL or the host callback) on rank- and round-dependent
// payloads of the per-iteration size; several rounds, so that both slots are reused.  *ok = 1 iff every round agreed and
// no wait ran out.  The caller combines the ranks' verdicts and switches the path off everywhere when any rank saw a
// difference (pmf_set_option("oneshot_allreduce", 0)): an all-reduce that has never run on the machine at hand does not
// get to carry the iteration on trust.
int pmf_ipc_selftest(pmf_ctx* c, int32_t rounds, int32_t* ok) {
  if (!c || !ok) return PMF_EINVAL;
  *ok = 0;
  if (c->ipc_nranks_ready <= 1) return fail(c, PMF_EINVAL, "pmf_ipc_selftest: no one-shot all-reduce set up (pmf_ipc_import)");
  if (!c->comm && !c->host_ar) return fail(c, PMF_EINVAL, "pmf_ipc_selftest: needs a second transport to compare with");
  if (!c->dIpcTestA || !c->dIpcTestB) return fail(c, PMF_EINVAL, "pmf_ipc_selftest: no test buffers (pmf_ipc_export allocates them)");
  const size_t count = std::min<size_t>((size_t)ps_elems(c), PMF_IPC_MAX_BYTES / sizeof(float));
  float *dA = c->dIpcTestA, *dB = c->dIpcTestB;
  std::vector<float> x(count), a(count), b(count);
  bool good = hipSetDevice(c->device) == hipSuccess;
  int rc = PMF_OK;
  c->ipc_wait_ticks = 2ull * 100000000ull;             // 2 s: the ranks enter the test together
  // EVERY rank runs EVERY round whatever it has seen so far: a rank that left early would leave its peers waiting in the
  // next round's collectives
  if (rounds < 2) rounds = 2;                          // (odd rounds run the split form the loop uses: never skipped)
  // the split form at THIS context's sizes: one flag per (P | S) tile of k_reduce_slabs_tiles, polled by every workgroup of
  // a consumer grid as large as launch_h_gram's
  const int ntu_ctx = c->NT * (c->np / 16) + c->NT * (c->NT + 1) / 2;
  const int nfl = ntu_ctx >= 1 && ntu_ctx <= PMF_IPC_MAX_WGS ? ntu_ctx : 74;   // (74: 64 bases x 256 columns)
  const int npull = std::max(1, std::min(c->np / 64, PMF_HGRAM_MAX_WGS));
  for (int t = 0; t < rounds; ++t) {
    for (size_t i = 0; i < count; ++i) x[i] = (float)((c->ipc.me + 1) * (t + 1)) + 0.001f * (float)(i % 977);
    const size_t cnt = t % 3 == 2 ? std::max<size_t>(1, count / 3) : count;      // (a shorter payload now and then)
    if (hipMemcpyAsync(dA, x.data(), cnt * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(dB, x.data(), cnt * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = PMF_EHIP; good = false; }
    c->ipc.nranks = c->ipc_nranks_ready;
    if (t & 1) {
      // the SPLIT form the loop uses (push inside a producer launch of many workgroups, wait + rank-ordered sum inside a
      // consumer launch): same slots, flags and sequence counter
      const unsigned seq = ++c->ipc_seq;
      hipLaunchKernelGGL(k_ipc_fold_push, dim3(nfl), dim3(256), 0, c->stream, dA, (int64_t)cnt, c->ipc, seq);
      hipLaunchKernelGGL(k_ipc_fold_pull, dim3(npull), dim3(1024), 0, c->stream, dA, (int64_t)cnt, c->ipc, seq, nfl, c->dIpcErr, c->ipc_wait_ticks);
      if (hipGetLastError() != hipSuccess) { rc = PMF_EHIP; good = false; }
      ++c->ipc_calls;
    } else if (allreduce_sum(c, dA, cnt, false) != PMF_OK) { rc = PMF_EHIP; good = false; }
    c->ipc.nranks = 0;                                 // the other transport
    if (allreduce_sum(c, dB, cnt, false) != PMF_OK) { rc = PMF_EHIP; good = false; }
    c->ipc.nranks = c->ipc_nranks_ready;
    if (hipMemcpyAsync(a.data(), dA, cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(b.data(), dB, cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { rc = PMF_EHIP; good = false; continue; }
    if (ipc_check(c) != PMF_OK) good = false;
    for (size_t i = 0; i < cnt && good; ++i)
      if (!(std::fabs(a[i] - b[i]) <= 1e-5f * std::fabs(b[i]))) good = false;
  }
  c->ipc_wait_ticks = PMF_IPC_WAIT_TICKS;
  (void)rc;                                            // (a failing call is a failed test, not an error of this function)
  *ok = good ? 1 : 0;
  return PMF_OK;
}

const char* pmf_collective_name(pmf_ctx* c) {
  if (!c) return "";
  static thread_local std::string s;
  const bool ipc = c->ipc.nranks > 1;
  s = ipc ? "one-shot IPC all-reduce (payloads <= 256 KiB: every rank writes into every peer's receive area, sums in rank order)" : "";
  if (c->comm) s += std::string(ipc ? " + " : "") + "ncclAllReduce (RCCL)" + (ipc ? " for larger payloads" : "");
  if (c->host_ar) s += std::string(s.empty() ? "" : " + ") + "host transport (pmf_set_host_allreduce)" + (ipc ? " for larger payloads" : "");
  if (s.empty()) s = "none";
  char buf[160];
  snprintf(buf, sizeof(buf), " [calls: ipc %lld (%lld of them folded into the slab-reduce / H-step launches), rccl %lld, host %lld]",
           (long long)c->ipc_calls, (long long)c->fold_calls, (long long)c->rccl_calls, (long long)c->host_calls);
  s += buf;
  return s.c_str();
}

// The caller changed V behind the library's back (a streamed `data` object was rebound or edited): forget
// everything derived from it -- ||V||^2, (W^T V | W^T W), the cached V H^T.
int pmf_invalidate_v(pmf_ctx* c) {
  if (!c) return PMF_EINVAL;
  v_replaced(c);
  return PMF_OK;
}

int pmf_snapshot_w(pmf_ctx* c) {
  PMFCHK(svd_csr_refuse(c, "pmf_snapshot_w"));
  PMFCHK(greedy_csr_refuse(c, "pmf_snapshot_w"));
  PMFCHK(cluster_csr_refuse(c, "pmf_snapshot_w"));
  PMFCHK(need(c, false, true, false));
  PMFCHK(materialize_w(c));
  if (!c->dWsnap) PMFCHK(dalloc_raw(c, &c->dWsnap, (size_t)c->mp * c->KP));
  HIPCHK(c, hipMemcpyAsync(c->dWsnap, c->dW, (size_t)c->mp * c->KP * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  c->wsnap_valid = true;
  return PMF_OK;
}

int pmf_restore_w(pmf_ctx* c) {
  if (!c) return PMF_EINVAL;
  if (!c->wsnap_valid) return fail(c, PMF_EINVAL, "pmf_restore_w: no snapshot (pmf_snapshot_w)");
  HIPCHK(c, hipSetDevice(c->device));
  PMFCHK(w_pipe_join(c));
  HIPCHK(c, hipMemcpyAsync(c->dW, c->dWsnap, (size_t)c->mp * c->KP * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  w_replaced(c, /*by_caller=*/false);
  if (c->dSing) HIPCHK(c, hipMemsetAsync(c->dSing, 0, sizeof(int), c->stream));
  return PMF_OK;
}

// H with the state derived from it: for NMF / BNMF the Gram matrix G = H H^T as the last H step left it (whole, or as the
// per-workgroup partial sums the next one-pass launch adds) -- a restored H then continues with the SAME bits of G; the other
// classes form G from H whenever they need it.
int pmf_snapshot_h(pmf_ctx* c) {
  PMFCHK(svd_csr_refuse(c, "pmf_snapshot_h"));
  PMFCHK(greedy_csr_refuse(c, "pmf_snapshot_h"));
  PMFCHK(cluster_csr_refuse(c, "pmf_snapshot_h"));
  PMFCHK(need(c, false, false, true));
  const size_t hb = (size_t)c->KP * c->np * sizeof(float), gb = (size_t)c->KP * c->KP * sizeof(float);
  if (!c->dHsnap) PMFCHK(dalloc_raw(c, &c->dHsnap, (hb + gb + (size_t)PMF_HGRAM_MAX_WGS * gb) / sizeof(float)));
  HIPCHK(c, hipMemcpyAsync(c->dHsnap, c->dH, hb, hipMemcpyDeviceToDevice, c->stream));
  if (c->dHd) {                    // SNMF: the float64 H with it (a restored H continues with the same bits)
    if (!c->dHdSnap) PMFCHK(dalloc_raw(c, &c->dHdSnap, 2 * hb / sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->dHdSnap, c->dHd, 2 * hb, hipMemcpyDeviceToDevice, c->stream));
  }
  const bool keep_g = (c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_BNMF) && c->g_valid && c->dG != nullptr;
  c->hsnap_g_valid = keep_g;
  c->hsnap_g_parts = keep_g ? c->g_parts : 0;
  if (keep_g) {
    char* gs = reinterpret_cast<char*>(c->dHsnap) + hb;
    HIPCHK(c, hipMemcpyAsync(gs, c->dG, gb, hipMemcpyDeviceToDevice, c->stream));
    if (c->g_parts > 0 && c->dGpart)
      HIPCHK(c, hipMemcpyAsync(gs + gb, c->dGpart, (size_t)c->g_parts * gb, hipMemcpyDeviceToDevice, c->stream));
  }
  c->hsnap_valid = true;
  return PMF_OK;
}

int pmf_restore_h(pmf_ctx* c) {
  if (!c) return PMF_EINVAL;
  if (!c->hsnap_valid) return fail(c, PMF_EINVAL, "pmf_restore_h: no snapshot (pmf_snapshot_h)");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t hb = (size_t)c->KP * c->np * sizeof(float), gb = (size_t)c->KP * c->KP * sizeof(float);
  HIPCHK(c, hipMemcpyAsync(c->dH, c->dHsnap, hb, hipMemcpyDeviceToDevice, c->stream));
  if (c->dHd && c->dHdSnap) HIPCHK(c, hipMemcpyAsync(c->dHd, c->dHdSnap, 2 * hb, hipMemcpyDeviceToDevice, c->stream));
  h_replaced(c, false, c->hd_force);   // (the float64 H was put back beside it, bit for bit: nothing new to widen)
  if (c->hsnap_g_valid) {
    const char* gs = reinterpret_cast<const char*>(c->dHsnap) + hb;
    HIPCHK(c, hipMemcpyAsync(c->dG, gs, gb, hipMemcpyDeviceToDevice, c->stream));
    if (c->hsnap_g_parts > 0)
      HIPCHK(c, hipMemcpyAsync(c->dGpart, gs + gb, (size_t)c->hsnap_g_parts * gb, hipMemcpyDeviceToDevice, c->stream));
    c->g_valid = true; c->g_parts = c->hsnap_g_parts;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

int pmf_kernel_exec_flops(pmf_ctx* c, double* executed_flops_per_launch) {
  if (!c || !executed_flops_per_launch) return PMF_EINVAL;
  *executed_flops_per_launch = c->stat.exec_flops;
  return PMF_OK;
}

int pmf_kernel_launch_ms(pmf_ctx* c, double* out_ms, int64_t cap, int64_t* count) {
  if (!c || (cap > 0 && !out_ms)) return PMF_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t pairs = (int64_t)(c->stat.used / 2);
  for (int64_t q = 0; q < pairs && q < cap; ++q) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->stat.ev[2 * q], c->stat.ev[2 * q + 1]));
    out_ms[q] = ms;
  }
  if (count) *count = pairs;
  return PMF_OK;
}

int pmf_abort(pmf_ctx* c, int32_t on) {
  if (!c) return PMF_EINVAL;
  c->abort_flag.store(on ? 1 : 0, std::memory_order_relaxed);
  return PMF_OK;
}

int pmf_synchronize(pmf_ctx* c) {
  if (!c) return PMF_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

}  // extern "C"
