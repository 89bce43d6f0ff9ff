/*
 * pymf_hip.h -- C ABI of libpymf_hip.so: the MI355X (gfx950) implementation of the
 * iterative factorize() hot path of nils-werner/pymf (NMF / NMFALS / SNMF).
 *
 * Plain C, no C++ or torch types.  One pmf_ctx drives ONE GPU from one host
 * thread (thread-compatible, not thread-safe); multi-GPU = one process (ctx)
 * per GPU, rows of V/W sharded, ONE cross-rank sum of (W^T V | W^T W) per iteration
 * inside pmf_factorize (for the single hooks: inside whichever of pmf_update_w /
 * pmf_update_h forms those sums -- all ranks make the same calls in the same order).
 * How that sum travels: for 2..8 ranks of one node, once
 * pmf_ipc_export / pmf_ipc_import have mapped the peers' receive areas and pmf_ipc_selftest
 * has agreed with the other transport on every rank, a ONE-SHOT exchange -- every rank writes
 * its partial into every peer's memory and adds the N partials in rank order -- folded into
 * the slab-reduce and H-step launches of the loop (no launch of its own); otherwise, and for
 * payloads beyond 256 KiB, ncclAllReduce on the context's RCCL communicator (or the host
 * callback of pmf_set_host_allreduce where the ranks cannot form one).  Every transport adds
 * in rank order: H stays bit-identical across the ranks.  The caller owns every host buffer;
 * the library owns all device memory, its HIP stream and its RCCL communicator.
 *
 * Reference interface each entry point replaces (paths into nils-werner/pymf):
 *   pmf_ctx_create        NMF.__init__                 pymf/nmf.py:71-97
 *   pmf_set_v_*           self.data (aliased ndarray)  pymf/nmf.py:93,123,129 (data[:,:])
 *   pmf_set_w/h, get_w/h  self.W / self.H attributes   pymf/nmf.py:116-120,173-177
 *   pmf_update_w          NMF.update_w                 pymf/nmf.py:128-132
 *                         SNMF.update_w                pymf/snmf.py:67-70
 *                         NMFALS.update_w              pymf/nmfals.py:85-97
 *   pmf_update_h          NMF.update_h                 pymf/nmf.py:122-126
 *                         SNMF.update_h                pymf/snmf.py:72-91
 *                         NMFALS.update_h              pymf/nmfals.py:70-82
 *                         BNMF.update_w / update_h     pymf/bnmf.py:79-90 (algo 3, 'next' row)
 *   pmf_frobenius         NMF.frobenius_norm           pymf/nmf.py:100-114
 *   pmf_factorize         NMF.factorize loop body      pymf/nmf.py:182-202
 *                         (incl. NMF.converged         pymf/nmf.py:134-139)
 *   pmf_rnmf_update_s     RNMF.update_s                pymf/rnmf.py:96-98   (algo 4, 'next' row)
 *   pmf_nndsvd_init       NNDSVD.update_w + SVD        pymf/nndsvd.py:78-106, pymf/svd.py:105-148
 *   pmf_stream_*          the data[:,:] reads of       pymf/nmf.py:123,129 for data that is not resident
 *   pmf_cnmf_init         CNMF.init_h + Kmeans         pymf/cnmf.py:78-103, pymf/kmeans.py:64-87 (algo 5)
 *   pmf_set/get_g_f64     self.G of CNMF               pymf/cnmf.py:95-100
 *   pmf_cluster_get/set_assigned  self.assigned of Kmeans  pymf/kmeans.py:77 (algo 6)
 *   pmf_sivm_get_select   self.select of SIVM          pymf/sivm.py:145-166,193 (algo 10)
 *   pmf_update_w under "sivm_rule" 1 / 2  LAESA.update_w / GMAP.update_w  pymf/laesa.py:63-82 / pymf/gmap.py:119-165 (algo 10)
 *   pmf_sivm_select       SIVM_CUR.sample              pymf/sivm_cur.py:65-73 (algo 10 or 14)
 *   pmf_svd_decompose / pmf_svd_get  SVD.factorize, U / S / V  pymf/svd.py:110-158 (algo 12; PCA: pymf/pca.py)
 *   pmf_cur_sqnorms       CUR.sample_probability       pymf/cur.py:84-97 (algo 14)
 *   pmf_cur_compute / pmf_cur_get  CUR.computeUCR, C / U / R  pymf/cur.py:99-120 (CMD: pymf/cmd.py)
 *   pmf_cur_ferr          CUR.frobenius_norm on sparse data  pymf/svd.py:92-107
 *   pmf_cur_leverage      CURSL.sample_probability     pymf/cursl.py:65-91 (algo 14)
 *   pmf_greedy_select     self.select of GREEDY        pymf/greedy.py:105-158 (algo 15; GREEDYCUR.sample: pymf/greedycur.py:62-68)
 *   pmf_vq_columns / pmf_vq_assign  vq, pdist            pymf/dist.py:107-130 (any algo with dense resident data)
 *   pmf_set_v_gather_f32  self.data[:, idx] of SUB     pymf/sub.py:169,181 (any algo; the source holds dense resident data)
 *
 * Every function returns PMF_OK (0) or a negative status and never throws;
 * pmf_last_error() gives a human-readable message for the last failure.
 */
#ifndef PYMF_HIP_H
#define PYMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmf_ctx pmf_ctx;

enum {
  PMF_OK = 0,
  PMF_EINVAL = -1,   /* bad argument / unsupported shape / call order */
  PMF_EHIP = -2,     /* a HIP runtime call failed */
  PMF_ENCCL = -3,    /* an RCCL call failed */
  PMF_ENOMEM = -4,   /* device or host allocation failed */
  PMF_ESINGULAR = -5, /* SNMF: H H^T is singular (the reference's np.linalg.inv raises LinAlgError, snmf.py:69) */
  PMF_ENUMERIC = -6   /* an iteration with a fixed cap of rounds did not finish (SIVM, AA: the multiplier search of the H step; AA: the rounds of the W step) */
};

enum { PMF_ALGO_NMF = 0, PMF_ALGO_NMFALS = 1, PMF_ALGO_SNMF = 2, PMF_ALGO_BNMF = 3, PMF_ALGO_RNMF = 4, PMF_ALGO_CNMF = 5,
       PMF_ALGO_KMEANS = 6, PMF_ALGO_CMEANS = 8, PMF_ALGO_SIVM = 10, PMF_ALGO_AA = 11, PMF_ALGO_PCA = 12 };   /* 7 and 9 are not assigned: pmf_ctx_create refuses them */
enum { PMF_ALGO_CUR = 14 };   /* CUR / CMD; 13 is not assigned and refused as well */
enum { PMF_ALGO_GREEDY = 15 };   /* GREEDY (and, through pmf_greedy_select on a CUR context, GREEDYCUR) */

/* pmf_factorize flags (the reference's factorize() keyword arguments, nmf.py:141-142) */
enum { PMF_COMPUTE_W = 1u, PMF_COMPUTE_H = 2u, PMF_COMPUTE_ERR = 4u };

#define PMF_NCCL_ID_BYTES 128

/* Number of visible HIP devices. */
int pmf_device_count(int32_t* out);

/* Fill out[PMF_NCCL_ID_BYTES] with a fresh RCCL unique id (call on rank 0, hand the
 * bytes to every rank by any means, then pass them to pmf_ctx_create). */
int pmf_nccl_unique_id(void* out);

/*
 * Create a context on HIP device `device`.
 *   algo      PMF_ALGO_*
 *   m_local   rows of V (= rows of W) held by THIS rank (the whole matrix when nranks==1)
 *   n         columns of V (= columns of H), identical on all ranks
 *   k         num_bases, 1 .. 2432 (NMFALS / NMFNNLS: 1 .. 1024); beyond 128 -- 64 for NMFALS -- generic kernels run.
 *             (The reference has no limit, nmf.py:116-120; beyond these PMF_EINVAL.)
 *   rank,nranks,nccl_id   RCCL world; nranks==1 -> nccl_id may be NULL and RCCL is not touched
 *                         (a non-NULL id with nranks==1 creates a 1-rank communicator)
 *                         With nranks > 1 the ranks must agree on which cached sums are current -- they decide which
 *                         collectives the next call runs: when ANY rank has uploaded new V, W or H (pmf_set_*), EVERY rank
 *                         calls pmf_invalidate_v before the next update / factorize / frobenius call (the host classes
 *                         exchange one flag per call for this, pymf_amd/nmf.py _sync_to_device).
 */
int pmf_ctx_create(pmf_ctx** out, int32_t algo, int64_t m_local, int64_t n, int32_t k,
                   int32_t device, int32_t rank, int32_t nranks, const void* nccl_id);
int pmf_ctx_destroy(pmf_ctx* ctx);
const char* pmf_last_error(const pmf_ctx* ctx);   /* ctx may be NULL: last create error */

/* V: host row-major m_local x n float32 with leading dimension ld (elements). Copied. */
int pmf_set_v_dense_f32(pmf_ctx* ctx, const float* V, int64_t ld);
/* V as CSR (m_local rows): indptr[m_local+1] int64, indices[nnz] int32, vals[nnz] f32.  Copied.  Semantics: the dense
 * algorithm on the matrix these arrays describe (entries of one (row, column) pair add up); pmf_frobenius and
 * PMF_COMPUTE_ERR refuse CSR data (PCA / SVD and GREEDY contexts excepted, below).  SNMF, NMF, CUR / CMD, PCA / SVD and GREEDY
 * contexts only; every other family returns PMF_EINVAL.
 * All check the arrays on the host before anything is uploaded (indptr from 0 to nnz and not decreasing, indices in
 * [0, n); the entries of a row may come in any order and repeat): malformed input is PMF_EINVAL and leaves the resident data
 * as it was.  pmf_check_csr: the same check of the arrays alone, for an m x n matrix, without a context or a device (the
 * message through pmf_last_error(NULL)).
 *   SNMF: num_bases > 128, or n * KP * 4 bytes beyond 160 KiB, expands the rows to a dense V on the device.
 *   NMF:  never a dense V.  The call builds the CSR arrays of V^T on the host by a stable counting sort and uploads them beside the rows; both half
 *         steps then run one gather-form kernel on stored entries (pmf_path_name: "nmf_csr_gather<NT>"), with the
 *         same bits on every run.  PMF_EINVAL, the message naming the limit, for num_bases > 128 and for more than
 *         one rank (nranks > 1, or a host / IPC transport installed).  pmf_stream_* refuses while CSR data is resident.
 *   CUR / CMD (algo 14): never a dense V.  Beyond the check above the column indices must ascend strictly within a row (a
 *         repeated entry would make the norms (a + b)^2 instead of a^2 + b^2): PMF_EINVAL otherwise.  The call builds the CSR
 *         arrays of V^T as for NMF, uploads both images and releases a resident dense V; a later dense upload releases the
 *         sparse arrays.  pmf_path_name: "cur_csr".  One rank only.  pmf_cur_sqnorms, pmf_cur_compute, pmf_cur_get and
 *         pmf_cur_ferr work on the stored entries; pmf_cur_leverage, pmf_frobenius, pmf_factorize (PMF_COMPUTE_ERR included),
 *         pmf_greedy_select, pmf_sivm_select and pmf_stream_* return PMF_EINVAL while CSR data is resident, and say so.
 *   PCA / SVD (algo 12): never a dense V.  The checks, the
 *         transposed copy and the release of a resident dense V are CUR / CMD's, strictly ascending columns included; on top of
 *         them min(rows, cols) padded to 64 must not exceed 1024 (the slab scheme of k_csr_gram).  pmf_path_name: "svd_csr".
 *         One rank only.  pmf_svd_decompose, pmf_svd_rank, pmf_svd_get, pmf_update_w, pmf_update_h, pmf_factorize and
 *         pmf_frobenius work on the stored entries (see "PCA / SVD" below); W and H are float64 on the device and travel through
 *         pmf_set_w_* / pmf_get_w_* / pmf_set_h_* / pmf_get_h_*.  pmf_stream_*, pmf_nndsvd_init, pmf_fill_w_uniform,
 *         pmf_fill_h_uniform, pmf_snapshot_w and pmf_snapshot_h return PMF_EINVAL while CSR data is resident, and say so.  A later
 *         dense upload releases the sparse arrays and the float64 factors (W and H are then unset).
 *   GREEDY (algo 15): never a dense V.  The checks (strictly ascending columns, one rank, min(rows, cols) padded to 64 at most
 *         1024), the transposed copy and the release of a resident dense V are PCA / SVD's.  pmf_path_name: "greedy_csr".
 *         pmf_update_w, pmf_update_h, pmf_factorize (PMF_COMPUTE_ERR included), pmf_frobenius, pmf_greedy_select (either side),
 *         pmf_sivm_get_select and the factor transfers work on the stored entries (see "GREEDY" below).  pmf_stream_*,
 *         pmf_nndsvd_init, pmf_fill_w_uniform, pmf_fill_h_uniform, pmf_snapshot_w and pmf_snapshot_h return PMF_EINVAL while CSR
 *         data is resident, and say so.  A later dense upload releases the sparse arrays and keeps W and H.
 *   Kmeans / Cmeans (algos 6, 8): never a dense V.  The checks (strictly ascending columns, one rank) and the transposed copy are
 *         CUR / CMD's; a resident dense V and the slabs of the dense pass are released.  pmf_path_name: "cluster_csr".
 *         pmf_update_w, pmf_update_h, pmf_factorize (PMF_COMPUTE_ERR included), pmf_frobenius, pmf_cluster_get_assigned,
 *         pmf_cluster_set_assigned and the factor transfers work on the stored entries (see "Kmeans / Cmeans" below).
 *         pmf_stream_*, pmf_nndsvd_init, pmf_fill_w_uniform, pmf_fill_h_uniform, pmf_snapshot_w and pmf_snapshot_h return
 *         PMF_EINVAL while CSR data is resident, and say so.  A later dense upload releases the sparse arrays and keeps W, H
 *         (rounded to float32) and the assignment. */
int pmf_set_v_csr_f32(pmf_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                      const float* vals, int64_t nnz);
int pmf_check_csr(int64_t m, int64_t n, const int64_t* indptr, const int32_t* indices, int64_t nnz);
/* V as CSC (n columns): indptr[n+1] int64, indices[nnz] int32 (row ids, ascending within a column, no duplicates), vals[nnz]
 * f32.  Copied.  SIVM contexts (algo 10) under "sivm_rule" 0 (SIVM) or 1 (LAESA) only -- the reference's own sparse branch
 * (pymf/sivm.py:110-120, pymf/dist.py:37-42); every other context, and a SIVM context under "sivm_rule" 2, "sivm_sgreedy" or
 * "sivm_gsat", returns PMF_EINVAL.  So does malformed input, checked on the host before anything is uploaded: indptr not from
 * 0 to nnz or decreasing, a row id outside [0, m), unsorted or duplicate rows in a column.  Semantics: the dense algorithm on
 * the matrix the arrays describe (stored zeros are entries like any other), computed from the stored entries alone: no dense V
 * exists on the device (a CSC upload releases one, a dense upload releases the CSC arrays).  pmf_update_w runs
 * k_sivm_csc_pass (pmf_sivm_csc.h; pmf_path_name: "sivm_csc_teams<TEAM>", TEAM the lanes per column of the next W step), pmf_update_h forms W^T V from the stored entries and
 * then runs the dense H step; H and W are dense.  A column measured against itself has distance exactly 0 under l2 and l1, as
 * on dense data.  While CSC data is resident pmf_frobenius, PMF_COMPUTE_ERR, pmf_sivm_select, pmf_gsat_* and a W step under a
 * rule other than SIVM or LAESA refuse (PMF_EINVAL, with a message); pmf_stream_* refuses SIVM contexts anyway.
 * pmf_set_option "sivm_csc_team" (0 default: by the mean stored entries per column; 4, 16, 64) forces the lanes that share a
 * column in k_sivm_csc_pass: the summation order, and so the last bits of a distance, depend on it and on nothing else.
 * pmf_check_csc: the same check of the arrays alone, for an m x n matrix, without a context or a device (the message through
 * pmf_last_error(NULL)). */
int pmf_set_v_csc_f32(pmf_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                      const float* vals, int64_t nnz);
int pmf_check_csc(int64_t m, int64_t n, const int64_t* indptr, const int32_t* indices, int64_t nnz);
/* Fill V on the device with the bench's synthetic U[0,1) stream (counter-based, so
 * the values depend only on (seed, global row, column)); row0 = first global row. */
int pmf_fill_v_uniform(pmf_ctx* ctx, uint64_t seed, int64_t row0);

/* The same for a float64 host array (the reference's default dtype, nmf.py:117,120): the bytes go up as they are and are
 * rounded to the device's float32 ON the device (no host-side conversion pass). */
int pmf_set_v_dense_f64(pmf_ctx* ctx, const double* V, int64_t ld);

/* W: m_local x k row-major (ld = k).  H: k x n row-major (ld = n). Host buffers. */
int pmf_set_w_f32(pmf_ctx* ctx, const float* W);
int pmf_get_w_f32(pmf_ctx* ctx, float* W);
int pmf_set_h_f32(pmf_ctx* ctx, const float* H);
int pmf_get_h_f32(pmf_ctx* ctx, float* H);
/* ... and for float64 host arrays -- what self.W / self.H are by default (nmf.py:117,120): rounded to / widened from the
 * device's float32 on the device, so that neither direction needs a conversion pass over m x k on the host.
 * SNMF with num_bases <= 128: H is KEPT in float64 on the device -- pmf_set_h_f64 / pmf_get_h_f64 carry the float64
 * values as they are; pmf_get_h_f32 returns their rounding, a float32 upload replaces them by the widened values. */
int pmf_set_w_f64(pmf_ctx* ctx, const double* W);
int pmf_get_w_f64(pmf_ctx* ctx, double* W);
int pmf_set_h_f64(pmf_ctx* ctx, const double* H);
int pmf_get_h_f64(pmf_ctx* ctx, double* H);
int pmf_fill_w_uniform(pmf_ctx* ctx, uint64_t seed, int64_t row0);
int pmf_fill_h_uniform(pmf_ctx* ctx, uint64_t seed);

/* One hook each (blocking until done on the device).  On shapes the one-pass kernel takes,
 * pmf_update_w also leaves (W^T V | W^T W) of the new W cached for the pmf_update_h that follows. */
int pmf_update_w(pmf_ctx* ctx);
int pmf_update_h(pmf_ctx* ctx);
int pmf_frobenius(pmf_ctx* ctx, double* out);   /* sqrt(sum((V - W H)^2)), all ranks' rows */

/*
 * The factorize() loop: for i in [0,niter): [update_w] [update_h] [ferr[i] = frobenius]
 * and, when PMF_COMPUTE_ERR and i > 1, stop if |ferr[i]-ferr[i-1]|/n < conv_eps
 * (nmf.py:134-139,198-202).  On convergence at iteration i, *converged_at = i
 * (the caller truncates ferr to ferr[:i] as the reference does) else -1.
 * *iters_done = number of loop bodies executed.  ferr may be NULL without PMF_COMPUTE_ERR.
 * Blocks until the device loop has finished.
 */
int pmf_factorize(pmf_ctx* ctx, int32_t niter, uint32_t flags, double conv_eps,
                  double* ferr, int32_t* iters_done, int32_t* converged_at);

/* BNMF only (pymf/bnmf.py:79-90,118-119): the penalty weights _lamb_W/_lamb_H used by the next
 * update_w/update_h; every update_h multiplies both by 1.1 (bnmf.py:84-85), as the reference does.
 * The caller sets 1/niter before each factorize() like BNMF.factorize. */
int pmf_set_lambda(pmf_ctx* ctx, double lamb_w, double lamb_h);
int pmf_get_lambda(pmf_ctx* ctx, double* lamb_w, double* lamb_h);

/* RNMF only (pymf/rnmf.py, algo 4; pmf_set_lambda(ctx, lamb, 0) sets the soft threshold _lamb):
 * pmf_rnmf_update_s = RNMF.update_s (rnmf.py:96-98), S = soft_thresholding(data - W H, lamb);
 * update_h runs it itself afterwards as the reference does (rnmf.py:107).  pmf_rnmf_get_s_f32
 * copies S (m_local x n, row-major) to the host. */
int pmf_rnmf_update_s(pmf_ctx* ctx);
int pmf_rnmf_get_s_f32(pmf_ctx* ctx, float* S);
/* S [m][n] contiguous handed to a context (the reference's S is an attribute that copies and pickles of the object carry,
 * rnmf.py:96-98; new data keeps it too: pmf_set_v_* on an RNMF context re-bases the device state D = S - data). */
int pmf_rnmf_set_s_f32(pmf_ctx* ctx, const float* S);

/* Streamed V (the `data[:, :]` idiom of nmf.py:123,129 for data that does not fit
 * in HBM: an h5py dataset, a memmap, a matrix beyond 288 GB).  NMF, BNMF, SNMF and NMFALS contexts (not RNMF: the reference's RNMF keeps S, an in-memory array of data's shape, rnmf.py:94-98); pmf_set_v_* is not
 * called.  One pass = one iteration of the reference loop (nmf.py:183-202):
 *   pmf_stream_begin(ctx, flags, max_tile_rows)   flags as pmf_factorize (PMF_COMPUTE_W/H/ERR)
 *   pmf_stream_tile(ctx, row0, rows, tile, ld)    row tiles in order; row0 and rows multiples of 64
 *                                                 (the last tile may be ragged); `tile` is row-major
 *                                                 host memory that must stay valid until the next but
 *                                                 one pmf_stream_tile call (or pmf_stream_end) has RETURNED:
 *                                                 the call waits for the copy of the tile two calls back
 *   pmf_stream_end(ctx, &ferr, &needs_direct)     H step; ferr = ||V - W H|| by the trace identity
 * needs_direct = 1 reports that the identity cancels (residual energy below 1e-3 of ||V||^2): a pass with
 * flags = PMF_STREAM_RESID evaluates sum((V - W H)^2) tile by tile instead (no update). */
#define PMF_STREAM_RESID 8u
int pmf_stream_begin(pmf_ctx* ctx, uint32_t flags, int64_t max_tile_rows);
int pmf_stream_tile(pmf_ctx* ctx, int64_t row0, int64_t rows, const float* tile, int64_t ld);
int pmf_stream_end(pmf_ctx* ctx, double* ferr, int32_t* needs_direct);

/* NNDSVD initialisation (pymf/nndsvd.py:79-108 = NNDSVD.update_w, with the SVD of pymf/svd.py:125-148):
 * fills the context's W and H from the dense V already set.  Needs n <= 16384 (the Gram matrix
 * data^T data is n x n: all its eigenpairs by a float64 Jacobi iteration up to 1024 columns, the num_bases largest
 * by a Chebyshev-filtered subspace iteration on the float64 MFMA beyond -- option "nndsvd_topk"; a wide matrix is handled by the caller on the transposed problem, as the
 * reference's SVD switches between its left and right forms, svd.py:237-246) and num_bases <= n.
 * rank_found (may be NULL) receives how many of the leading num_bases eigenvalues exceed the
 * reference's 1e-8 cut (svd.py:130-131); fewer than num_bases is PMF_EINVAL (the reference raises
 * IndexError).  Row-sharded contexts sum the Gram matrix and the split norms over all ranks. */
int pmf_nndsvd_init(pmf_ctx* ctx, int32_t* rank_found);

/* CNMF (algo 5; pymf/cnmf.py, convex NMF: W = data G, H >= 0, G >= 0; dense data, n <= 4096, num_bases <= 128, num_bases <= n,
 * one rank -- pmf_ctx_create returns PMF_EINVAL otherwise).  The whole loop runs in Gram space on C = V^T V (n x n, float64,
 * formed once per V); G (n x k) and H are kept in float64 on the device.  With algo 5 the common entry points mean:
 *   pmf_set_h_f64 / pmf_get_h_f64   the float64 H as it is (exact round trip)
 *   pmf_factorize                   cnmf.py:156-187 under the PMF_COMPUTE_* flags and conv_eps; one call, no host round trip per
 *                                   iteration while the error runs on the trace identity
 *   pmf_frobenius                   ||data - W H||: W = V G by the trace identity (the direct residual below 1e-3 of ||V||^2), or
 *                                   the direct residual with a W the caller uploaded (pmf_set_w_*) until a G step rebinds W
 *   pmf_get_w_*                     V G for the current G (materialised once), or the caller's W
 *   pmf_update_w / pmf_update_h     no-ops, as cnmf.py:70-76
 * pmf_cnmf_init = CNMF.init_h: Kmeans(data, num_bases).factorize(niter=km_niter) in Gram space from the centres data[:, sel]
 * (sel: num_bases sorted distinct sample indices -- what random.sample drew, kmeans.py:71-74), then H = onehot^T + 0.2 and,
 * unless G has been set, G = (onehot + 0.01) / count (cnmf.py:88-100); W = V G unless W was set.  assigned_out (may be NULL):
 * the n cluster indices.  pmf_set_g_f64 / pmf_get_g_f64: G as a host n x k row-major float64 array, exact round trip. */
int pmf_cnmf_init(pmf_ctx* ctx, const int32_t* sel, int32_t km_niter, int32_t* assigned_out);
int pmf_set_g_f64(pmf_ctx* ctx, const double* G);
int pmf_get_g_f64(pmf_ctx* ctx, double* G);

/* Kmeans (algo 6; pymf/kmeans.py) and Cmeans (algo 8; pymf/cmeans.py, fuzzifier m = 1.75): dense data, any m and n,
 * num_bases <= 128, one rank -- pmf_ctx_create returns PMF_EINVAL otherwise.  One pass over V per iteration, spread over
 * column panels of V (pmf_cluster.h); all cross-panel sums have a fixed order.  With these algos the common entry points mean:
 *   pmf_update_h     Kmeans: assigned = argmin_j ||v_c - w_j|| (lowest index on ties), H one-hot (kmeans.py:75-79);
 *                    Cmeans: H_jc = 1 / sum_i (d_jc / d_ic)^(2/(m-1)), d = ||v_c - w_j|| + 1e-8 (cmeans.py:71-81); needs V, W
 *   pmf_update_w     Kmeans: centres with more than one member become the mean of their members (kmeans.py:82-87; needs an
 *                    assignment: an H step, or pmf_cluster_set_assigned); Cmeans: W = V H^T / (rowsum(H) + 1e-8)
 *   pmf_factorize    nmf.py:182-202: update_w, update_h, ||V - W H||, the convergence rule, under the PMF_COMPUTE_* flags
 *   pmf_frobenius    the direct residual
 * pmf_cluster_get_assigned: the n cluster indices of the last Kmeans H step (or the ones set); pmf_cluster_set_assigned: a
 * caller's assignment (n indices in [0, num_bases)), which the next pmf_update_w uses.
 * On CSR data (pmf_set_v_csr_f32 on a Kmeans / Cmeans context; path "cluster_csr") both steps run on stored entries.  W stays
 * float32 [mp][KP]; H lives transposed in float64, H^T [np][64 or 128], and the H transfers transpose on the way.
 * pmf_update_h: k_cluster_csr_assign<NH, algo> -- a wave per sample (a line of the image of V^T), lane <-> centre,
 * d^2 = |v|^2 - 2 v.w + |w|^2 in float64 from exact products, argmin (lowest index on ties) or memberships, the denominators
 * as per-workgroup partials added in workgroup order.  pmf_update_w: k_cluster_csr_num<NH, algo> -- a wave per chunk of 512
 * stored entries of a data row (the chunks follow from indptr alone), Kmeans reading the assignment, Cmeans the rows of H^T --
 * and k_cluster_csr_finish, which adds a row's chunks in order, divides and rounds once to float32.  pmf_frobenius and the
 * error of pmf_factorize: Kmeans right behind its own H step sqrt(sum min d^2); otherwise the float64 identity
 * ||data||^2 - 2 <W^T data, H> + <W^T W, H H^T>, clamped at 0 before the root.  No atomics: two runs give the same bits.
 * pmf_profile_enable times both kernels; the record names the one launched last. */
int pmf_cluster_get_assigned(pmf_ctx* ctx, int32_t* assigned);
int pmf_cluster_set_assigned(pmf_ctx* ctx, const int32_t* assigned);

/* SIVM (algo 10; pymf/sivm.py, simplex volume maximisation: W = num_bases selected columns of the data, the columns of H on the
 * simplex): dense data, data_dimension <= 16384, num_bases <= 64, one rank -- pmf_ctx_create returns PMF_EINVAL otherwise.
 * pmf_set_option "sivm_metric" (0 'l2' default, 1 'l1', 2 'cosine') and "sivm_init" (0 'fastmap' default, 1 'origin') carry the
 * constructor's dist_measure and init.  With algo 10 the common entry points mean:
 *   pmf_update_w     SIVM.update_w (sivm.py:145-201): num_bases + 2 ('fastmap') or num_bases ('origin') passes over V enqueued
 *                    back to back (pmf_sivm.h), then W = V[:, select]; needs V only.  Two runs give the same bits.
 *   pmf_update_h     AA.update_h (aa.py:93-111): per column min 1/2 x^T W^T W x - (W^T v)^T x, x >= 0, sum x = 1, as rounds of
 *                    non-negative QPs with right-hand side W^T v + lambda and a bracketing secant on sum x(lambda) - 1; needs
 *                    V, W.  PMF_EINVAL when W^T W is not positive definite (H is not unique: duplicate selected columns, or
 *                    num_bases > data_dimension), PMF_ENUMERIC when a column is left with |sum x - 1| > 1e-6 after 48 rounds.
 *   pmf_factorize    update_w, update_h, ||V - W H|| under the PMF_COMPUTE_* flags; the class always passes niter = 1
 *   pmf_frobenius    the direct residual
 * pmf_sivm_get_select: the num_bases selected column indices of the last pmf_update_w in selection order; under 'origin' the
 * first is -1, which W treats as a Python index (the LAST data column, sivm.py:198).  GREEDY contexts (algo 15) answer it too.
 *
 * LAESA and GMAP run on the same context (no algorithm number of their own): pmf_set_option "sivm_rule" (0 SIVM default,
 * 1 LAESA, 2 GMAP) chooses the rule pmf_update_w selects by, "gmap_method" (0 'pca' default, 1 'aa', 2 'nmf') GMAP's method;
 * both options are refused (PMF_EINVAL) on other contexts and out of range.  Limits, pmf_update_h, pmf_factorize,
 * pmf_frobenius and pmf_sivm_get_select are SIVM's.
 *   sivm_rule 1      LAESA.update_w (pymf/laesa.py:63-82): the plain rounds of 'fastmap' / 'origin' as above, then num_bases - 1
 *                    rounds dmin = min(dmin, distance to the last selected column), select the argmax of dmin ("sivm_metric"
 *                    and "sivm_init" apply): num_bases + 2 / num_bases launches of k_laesa_pass (pmf_colsel.h).  Distances
 *                    fp32, dmin float64.
 *   sivm_rule 2      GMAP.update_w (pymf/gmap.py:119-165 with robust_map = False): round 0 the column norms and the first
 *                    argmax, then num_bases - 1 rounds c = v . x / (|v| |x|), iterval *= (1 - |c|) |v| ('pca'),
 *                    ((1 - c) / 2) |v| ('aa') or 1 - |c| ('nmf'), select the argmax of iterval: num_bases launches of
 *                    k_gmap_pass.  Sums of squares and dots fp32, norms and iterval float64.  A zero-norm column scores NaN
 *                    and is never selected (the reference's np.argmax would pick it).  The robust_map = True path of the
 *                    reference (a nested, randomly initialised Kmeans) is not provided.
 *
 * SIVM_SGREEDY (pymf/sivm_sgreedy.py:96-133, the exact greedy max-volume selection) runs on the same context under
 * pmf_set_option "sivm_sgreedy" (0 default, 1); the option is refused (PMF_EINVAL) on other contexts, out of range and together
 * with "sivm_rule" 1 or 2.  pmf_update_w then runs init_sivm's plain rounds ("sivm_metric" and "sivm_init" apply to them alone:
 * three launches of k_laesa_pass for 'fastmap', one for 'origin') and num_bases - 1 rounds of k_sgreedy_step and k_sgreedy_pass
 * (pmf_sgreedy.h): the Cayley-Menger volume of "selected + candidate" for every column from l2 distances, as
 * det(CM_S) (-b^T inv(CM_S) b) with the squared distances fp32 and everything behind them float64; the argmax joins the
 * selection.  pmf_sivm_get_select answers in the reference's order of `select` -- all but the last pick ascending, then the last
 * pick; under 'origin' the first entry is -1: the last data column is the first vertex -- and W's columns follow it.  Selections
 * are the reference's while the selected columns stay affinely independent (num_bases <= data_dimension + 1 on data in general
 * position); beyond that every volume is rounding noise in the reference too, and the indices returned are valid but arbitrary.
 * pmf_sivm_select keeps SIVM's rule on such a context.  Limits, pmf_update_h, pmf_factorize and pmf_frobenius are SIVM's.
 * pmf_sivm_get_volumes: the num_bases - 1 volumes of the rounds of the last pmf_update_w (the reference's _v), float64;
 * contexts under "sivm_sgreedy" only. */
int pmf_sivm_get_select(pmf_ctx* ctx, int32_t* select);
int pmf_sivm_get_volumes(pmf_ctx* ctx, double* volumes);

/* SIVM_GSAT (pymf/sivm_gsat.py:82-125, the online swap-based volume maximisation) runs on the same context under
 * pmf_set_option "sivm_gsat" (0 default, 1); the option is refused (PMF_EINVAL) on other contexts, out of range and together
 * with "sivm_rule" 1 or 2 or "sivm_sgreedy".  Under it pmf_update_w refuses: the vertices move through the entries below, which
 * keep W as the context's W (pmf_get_w_*, pmf_update_h, pmf_frobenius see every swap).  "sivm_metric" 0 'l2' or 1 'l1' is the
 * measure of the distances between a probe and the vertices; the distances among the vertices are l2 whatever it says, as the
 * reference mixes them; 2 'cosine' is refused.  Distances and volumes are float64 from the float32 values; pmf_gsat.h.
 * pmf_gsat_start: the walk's state from the context's W (its num_bases columns are the vertices; pmf_set_w_* first) and
 *   `select` (num_bases indices: the data column each vertex is, any value outside [0, num_samples) for a vertex that is none):
 *   the l2 distance table and V = cmdet of it (sivm_gsat.py:84-88); the log of volumes starts empty.  A state that belongs to
 *   the current W is kept (started = 0 on return) unless force != 0; pmf_set_w_* ends it.  Dense resident data, one rank.
 * pmf_gsat_walk: n probes, the data columns idx[0 .. n) in this order, each as sivm_gsat.py:119-125 with online_update_w
 *   behind it: slots_out[i] is the vertex that probe i replaced, -1 for a reject, -2 for a probe that was in `select` when its
 *   turn came.  Probes are evaluated 256 to a launch (k_gsat_probe) against the current vertices; the first accepted one is
 *   applied (k_gsat_commit) and the probes behind it are evaluated again, so the verdicts are those of the one-by-one
 *   sequence.  One 4-byte read per launch pair.  An index outside [0, num_samples) is PMF_EINVAL before anything runs.
 * pmf_gsat_probe_vec: online_update_w (sivm_gsat.py:82-117) on a vector of data_dimension floats that need not be a data
 *   column: slot_out is the vertex it replaced or -1; `select` is left as it is, as in the reference.
 * pmf_gsat_get_volumes: count = the entries of the reference's _v since pmf_gsat_start (0 before the first swap, then the
 *   volume before the first swap and every accepted volume), the first min(cap, count) of them into volumes (may be NULL
 *   with cap = 0), and V, the current volume.
 * pmf_gsat_get_d: the reference's D as it leaves it, (num_bases + 1)^2 float64 row-major: the distance table, in row and
 *   column num_bases the distances of the last probe that was evaluated (zeros before the first), the corner 0.
 * pmf_sivm_get_select answers with the walk's `select`.  Decisions are the reference's while num_bases <= data_dimension + 1
 * on data in general position; beyond that every volume is rounding noise in the reference too: slots and indices stay valid. */
int pmf_gsat_start(pmf_ctx* ctx, const int32_t* select, int32_t force, int32_t* started);
int pmf_gsat_walk(pmf_ctx* ctx, const int64_t* idx, int64_t n, int32_t* slots_out);
int pmf_gsat_probe_vec(pmf_ctx* ctx, const float* vec, int32_t* slot_out);
int pmf_gsat_get_volumes(pmf_ctx* ctx, double* volumes, int64_t cap, int64_t* count, double* V);
int pmf_gsat_get_d(pmf_ctx* ctx, double* D);

/* pmf_sivm_select: SIVM's selection alone (pymf/sivm_cur.py:65-73: what SIVM_CUR.sample asks of SIVM) on a SIVM or a CUR / CMD
 * context -- nsel indices in selection order among the columns of V (transposed = 0) or among its rows (transposed = 1: SIVM on
 * the transposed view), under metric 0 'l2', 1 'l1' or 2 'cosine' and init 0 'fastmap' or 1 'origin' (the first entry is then -1).
 * path 0 chooses the kernel by shape: columns run k_sivm_pass on V while rows <= 16384 and otherwise the long-sample pass
 * (k_sivm_rowdist, k_sivm_rowstep: pmf_sivm.h) on a transposed copy; rows run the long-sample pass on V itself, without a copy,
 * while rows <= 16384 and otherwise k_sivm_pass on the transposed copy.  path 1 forces k_sivm_pass, path 2 the long-sample pass,
 * each on a transposed copy where the layout needs one; PMF_EINVAL where the kernel's limit (samples of dimension <= 16384;
 * at most 16384 candidates) does not allow it.  All rounds are enqueued back to back; state and partials are temporaries of
 * the call: the context's own selection state, pmf_update_w and pmf_sivm_get_select are not touched.  Dense resident data, one
 * rank, 1 <= nsel <= 64, min(rows, cols) <= 16384 -- PMF_EINVAL otherwise.  Two calls give the same bits.
 * The rule is always SIVM's, whatever "sivm_rule" the context carries: SIVM_CUR depends on it.
 * pmf_set_option "profile_sivm_rows" (0 default, 1) makes pmf_profile_enable time the rounds of the long-sample pass. */
int pmf_sivm_select(pmf_ctx* ctx, int32_t transposed, int32_t nsel, int32_t metric, int32_t init, int32_t path, int32_t* select);

/* AA (algo 11; pymf/aa.py, archetypal analysis: column i of W is the projection of (data pinv(H))[:, i] onto the convex hull of
 * the data columns, W = data beta^T with beta >= 0 and rows summing to 1; the H step is the one SIVM inherits).  Dense resident
 * data, one rank, num_bases <= 64, min(data_dimension + 1, num_samples) <= 128 (a base's corral of data columns).
 *   pmf_update_w     AA.update_w (aa.py:113-134) as column generation (pmf_aa.h): W_hat through inv(H H^T) -- an H without full
 *                    row rank is PMF_EINVAL --, then rounds of one pricing pass over V and one master step per base; a first
 *                    batch of rounds is enqueued blind, then one counter is read per round; PMF_ENUMERIC when the cap of
 *                    rounds is reached.  Needs V and H.  Two runs give the same bits.
 *   pmf_update_h     AA.update_h (aa.py:93-111), as for SIVM.          pmf_frobenius: the direct residual.
 *   pmf_factorize    NMF.factorize's loop (W step, H step, error, convergence test) for any niter.
 * pmf_aa_get_beta: beta of the last pmf_update_w, num_bases x num_samples float64, row-major.
 * pmf_aa_rounds: the rounds that W step took. */
int pmf_aa_get_beta(pmf_ctx* ctx, double* beta);
int pmf_aa_rounds(pmf_ctx* ctx, int32_t* rounds);

/* CHNMF (pymf/chnmf.py; on an AA context with dense resident data, one rank): the columns on the convex hulls of pairwise random
 * projections, chnmf.py:154-183.
 * pmf_chnmf_hull: R is the projection matrix, base_sel x data_dimension float64, row-major, 2 <= base_sel <= min(16,
 *   data_dimension).  proj = R V is formed in float64 on the device (float64 MFMA, V widened on load) and stays there; for every
 *   pair of its rows (itertools.combinations order) a filter over all samples (extremes in 32 fixed directions, then every point
 *   inside their polygon by more than 64 2^-53 times the largest coordinate is discarded) and the exact hull of the survivors
 *   (sorted by (x, y, index); monotone chain with a strict turn test; of bit-identical points the lowest index) run back to back
 *   without a host round trip between pairs.  A pair with more than 4096 survivors is run again with 128 directions and, if that
 *   does not help, its hull is formed on the host from its two rows of proj: never truncated.  idx_out receives the union of all
 *   pairs' vertices, ascending (np.unique); *count_out their number; more than cap of them is PMF_EINVAL (*count_out is set).
 *   Every comparison that decides membership is float64; two runs give the same bits.
 * pmf_chnmf_set_limits [test reference]: the survivor capacity (0: 4096) and the largest number of workgroups of the sweeps
 *   (0: 1024; fewer make a workgroup own more 64-column panels) of the following pmf_chnmf_hull calls.
 * pmf_chnmf_routes: routes[0..2] = the pairs of the last pmf_chnmf_hull that ended on the 32-direction filter, on the
 *   128-direction rerun, on the host. */
int pmf_chnmf_hull(pmf_ctx* ctx, const double* R, int32_t base_sel, int32_t* idx_out, int64_t cap, int64_t* count_out);
int pmf_chnmf_set_limits(pmf_ctx* ctx, int32_t survivor_cap, int32_t max_wgs);
int pmf_chnmf_routes(pmf_ctx* ctx, int32_t* routes);

/* vq / pdist (pymf/dist.py:107-130) against the resident data: nq <= 128 query vectors of dimension data_dimension are measured
 * against EVERY data column in one sweep over V (k_vq_pass, pmf_vq.h).  Q is data_dimension x nq float32 on the host, query j's
 * component r at Q[r*ldq + j].  metric 0 'l2' = sqrtf(sum (v - q)^2), 1 'l1' = sum |v - q|, in fp32 from the difference, one
 * running sum per pair down the rows (dist.py:61, dist.py:33: no norm expansion, so data far from the origin lose nothing);
 * relative error of a distance at most (data_dimension + 4) 2^-24.
 * pmf_vq_columns: idx_out[j] = the data column nearest to query j, the lowest column among equally near ones (np.argmin);
 *   dist_out[j] (may be NULL) its distance.  A NaN distance never wins; a query whose distances are all NaN gets column 0 and
 *   the distance NaN.  Per workgroup and query one (distance, column) partial, reduced by k_vq_close: no float atomics.
 * pmf_vq_assign: idx_out[c] (num_samples entries; may be NULL) = the query nearest to data column c, the lowest query among
 *   equally near ones; dist_all (may be NULL; not both) = the whole block, nq x num_samples float64 row-major, dist_all[j*n + c]
 *   the fp32 distance of query j to column c, widened.  The block is written once by the sweep (a temporary of
 *   8 nq num_samples bytes on the device) and read once by k_vq_argmin_rows.
 * Both work on a context of ANY algo whose float32 V is resident and dense (pmf_set_v_dense_*, pmf_fill_v_uniform), one rank;
 * they read V only: factors, selections and caches stay as they are (like every entry they end the float64-H bookkeeping of the
 * previous call, as need() does).  The sweep parallelises over COLUMNS only -- one workgroup per 64-column panel at most -- so tall,
 * narrow data (a million rows by a few hundred columns) is correct but occupies few compute units.  PMF_EINVAL, with a
 * message, when the context holds CSR or CSC data, when no dense data is resident (streamed data never is), when nq < 1 or
 * nq > 128, when the metric is not 0 or 1.  Two calls give the same bits.
 * pmf_set_option "profile_vq" (0 default: the context's own kernel, 1: k_vq_pass, 2: k_vq_argmin_rows) chooses the launch that
 * pmf_profile_enable times, on any context. */
int pmf_vq_columns(pmf_ctx* ctx, const float* Q, int64_t ldq, int32_t nq, int32_t metric, int32_t* idx_out, double* dist_out);
int pmf_vq_assign(pmf_ctx* ctx, const float* Q, int64_t ldq, int32_t nq, int32_t metric, int32_t* idx_out, double* dist_all);

/* Column gather between contexts (SUB's sample, pymf/sub.py:169,181; k_gather_cols, pmf_gather.h): dst's dense float32 V becomes
 * src.V[:, idx[j]] for j < nsel, filled on the device -- the data of src do not cross the host link again.
 *   idx    nsel int64 column indices of src, in any order, repeats allowed; NULL: all columns in order (a whole copy), nsel must
 *          then equal src's n
 *   dst    src's m rows by nsel columns (nsel == dst's n), of ANY algo; src: any algo whose float32 V is resident and dense
 * The copy is exact to the bit (NaN payloads, infinities, -0.0); the pad of dst's image comes out zero, as a dense upload leaves
 * it.  Everything that follows a new V is what pmf_set_v_dense_f32 runs (the caches of the old V are dropped, ||V||^2 is enqueued,
 * CSR / CSC data of dst is released, RNMF keeps its S): a context filled this way cannot be told from one that was given the same
 * columns by pmf_set_v_dense_f32.  The two contexts keep their own streams, ordered by two events: what src's stream holds
 * completes before the kernel reads, and the kernel completes before work enqueued on src afterwards runs; the call does not wait
 * for the kernel on the host and never synchronises the device.  PMF_EINVAL with a message naming the condition (through
 * pmf_last_error(dst)), decided on the host before any launch and leaving dst's data and derived state as they were: an index < 0
 * or >= src's n; nsel != dst's n; different row counts; src without data; src holding CSR or CSC data or in streamed mode; src ==
 * dst; contexts on different devices; either context in a multi-rank world.
 * pmf_set_option(dst, "profile_gather", 1) makes k_gather_cols the launch that pmf_profile_enable times on dst (0: dst's own kernel).
 * pmf_get_v_dense_f32: the resident dense V, m x n, into out (host, row-major, leading dimension ld >= n elements); PMF_EINVAL when
 * no dense data is resident. */
int pmf_set_v_gather_f32(pmf_ctx* dst, pmf_ctx* src, const int64_t* idx, int64_t nsel);
int pmf_get_v_dense_f32(pmf_ctx* ctx, float* out, int64_t ld);

/* PCA / SVD (algo 12; pymf/svd.py:110-158 for dense data, pymf/pca.py): the SVD of the resident V through the eigen-decomposition
 * of its Gram matrix on the short side -- V^T V for rows > cols (_left_svd), V V^T otherwise (_right_svd) -- formed in float64
 * on the float64 MFMA (k_prod_f64, upper block triangle), decomposed by the float64 Jacobi solver of pmf_nndsvd_init.  Eigenvalues <= 1e-8 are dropped
 * as in svd.py, the rest sorted descending; the side that comes from the eigenvectors is float64, the projected side
 * (U = data V^T S^-1 or V = S^-1 U^T data) is multiplied in float32.  Dense resident data, one rank, min(rows, cols) <= 2432,
 * and the context's k >= min(rows, cols) (the largest possible rank; W and H are k wide) -- pmf_ctx_create returns PMF_EINVAL
 * otherwise.  pmf_set_option "pca_num_bases" (0 = all, the default) carries PCA's num_bases.  With algo 12:
 *   pmf_update_w     PCA.update_w (pca.py:93-108): the decomposition, then W = the leading pca_num_bases columns of U (the other
 *                    columns zero); needs V only.  Two runs give the same bits.
 *   pmf_update_h     PCA.update_h (pca.py:90-91): H = W^T V; needs V, W
 *   pmf_factorize    update_w, update_h, ||V - W H|| under the PMF_COMPUTE_* flags; the class always passes niter = 1
 *   pmf_frobenius    the direct residual
 * pmf_svd_decompose: the decomposition alone; *rank = the number of singular triples kept.  It leaves W = U and H = S V, so
 * that pmf_frobenius is svd.py's ||data - U S V||.
 * pmf_svd_get: U (rows x rank), S (rank values) and V (rank x cols) of the last decomposition as float64, row-major; a NULL
 * pointer skips that factor.  pmf_svd_rank: the rank of that decomposition (what a PCA W step found).  Both return PMF_EINVAL
 * when the resident V has not been decomposed.
 * On CSR data (pmf_set_v_csr_f32; path "svd_csr") the Gram matrix of the short side comes from the stored entries in exact fixed
 * point (k_csr_gram on the image of V for rows > cols, on the image of V^T otherwise), the solver, the cut and the order are the
 * same, and pmf_set_option "svd_num_triples" (0 = all, the default; at most 1024) cuts the kept triples to the leading ones: it
 * carries SVD's k and PCA's num_bases.  The projected side, PCA's H = W^T V and the cross term of the error are one float64 pass
 * over the stored entries (k_csr_proj_f64); every factor is float64.  pmf_frobenius is the trace identity
 * ||V||^2 - 2 <W^T V, H> + <W^T W, H H^T> in float64, clamped at 0 -- behind pmf_svd_decompose with W = U, H = S V, where
 * pmf_get_w_* / pmf_get_h_* refuse (pmf_svd_get reads the factors).  pmf_update_w with another number of bases than the resident
 * H has drops that H.  Two runs give the same bits. */
int pmf_svd_decompose(pmf_ctx* ctx, int32_t* rank);
int pmf_svd_rank(pmf_ctx* ctx, int32_t* rank);
int pmf_svd_get(pmf_ctx* ctx, double* U, double* S, double* V);

/* CUR / CMD (algo 14; pymf/cur.py, pymf/cmd.py for dense data): data ~ C U R with C = data[:, cid] diag(sqrt(ccnt)),
 * R = diag(sqrt(rcnt)) data[rid, :] and U = pinv(C) data pinv(R), computed as (C^T C)^+ (C^T data R^T) (R R^T)^+: the two small
 * Gram matrices and the middle product -- the one pass over the data -- are formed in float64 on the float64 MFMA (one kernel,
 * k_prod_f64, with two tile maps), the pseudo-inverses come from the float64 Jacobi solver with svd.py's cut (eigenvalues <= 1e-8 dropped).  Dense
 * resident data, one rank, the context's k = max(nr, nc) <= 128 -- PMF_EINVAL otherwise.  There are no W / H steps and no
 * pmf_factorize with algo 14.  Two runs give the same bits.
 * pmf_cur_sqnorms: the row sums (row_sq [m]) and column sums (col_sq [n]) of data^2 in float64, one read of V: what
 * CUR.sample_probability normalises (cur.py:84-97); the draws stay with the caller.  A NULL pointer skips that side.
 * pmf_cur_compute: CUR.computeUCR (cur.py:99-120) for nr row indices rid with multiplicities rcnt and nc column indices cid with
 * multiplicities ccnt, 1 <= nr, nc <= min(128, k); a negative index counts from the end (-1 is the last row / column), rcnt or
 * ccnt NULL means all ones; indices need not be sorted or distinct.  PMF_EINVAL for an index out of range or a count < 1.  It
 * leaves W = C U and H = R (float32), so that pmf_frobenius is svd.py's ||data - C U R||.
 * pmf_cur_get: C (m x nc), U (nc x nr) and R (nr x n) of the last pmf_cur_compute as float64, row-major, C and R scaled as
 * the reference returns them; a NULL pointer skips that factor.  PMF_EINVAL when the resident V has not been decomposed.
 * On CSR data (pmf_set_v_csr_f32) the three calls above read stored entries only: the norms by k_cur_csr_sqnorms, the gathers by
 * k_cur_csr_gather, the middle product by k_cur_csr_mid (walks the selected rows and their crossing columns, float64, chunk
 * partials added in a fixed order); Gram matrices, pseudo-inverses and the host finish are those of dense data.  C and R come
 * back dense.  Two runs give the same bits.
 * pmf_cur_ferr: CSR data only: *out = ||data - C U R||_F of the last pmf_cur_compute in float64, from the identity
 * ||data||^2 - 2 <U, C^T data R^T> + <(C^T C) U, U (R R^T)> (clamped at 0 before the root) on quantities that call formed:
 * no dense image.  PMF_EINVAL on dense data (pmf_frobenius is the error there) and before a pmf_cur_compute. */
int pmf_cur_sqnorms(pmf_ctx* ctx, double* row_sq, double* col_sq);
int pmf_cur_compute(pmf_ctx* ctx, const int32_t* rid, const int32_t* rcnt, int32_t nr, const int32_t* cid, const int32_t* ccnt, int32_t nc);
int pmf_cur_get(pmf_ctx* ctx, double* C, double* U, double* R);
int pmf_cur_ferr(pmf_ctx* ctx, double* out);

/* CURSL (pymf/cursl.py: CMD with statistical leverage scores as sampling probabilities) on a CUR / CMD context (algo 14).
 * pmf_cur_leverage: row_lev [m] = the squared row norms of the leading min(k_rows, rank) left singular vectors of the resident
 * data, col_lev [n] = the squared column norms of the leading min(k_cols, rank) right singular vectors, float64, unnormalised:
 * what CURSL.sample_probability divides by k and normalises (cursl.py:66-85; svd.py keeps the triples with an eigenvalue > 1e-8).
 * Each vector sums to its min(k, rank).  The eigenpairs of the float64 Gram matrix on the short side are cached per V and shared
 * with pmf_greedy_select; the long side is one read of V on the float64 MFMA (k_lev_f64), the projected singular vectors are
 * never written out.  A NULL pointer skips that side.  Dense resident data, one rank, k_rows, k_cols >= 1, min(k, rank) <= 128,
 * min(rows, cols) <= 2432 -- PMF_EINVAL otherwise.  Two calls give the same bits.
 * pmf_set_option "profile_cur" (0 default: the cross product of pmf_cur_compute, 1: k_lev_f64, 2: k_cur_sqnorms) chooses the
 * launch that pmf_profile_enable times on a CUR / CMD context. */
int pmf_cur_leverage(pmf_ctx* ctx, int32_t k_rows, int32_t k_cols, double* row_lev, double* col_lev);

/* GREEDY (algo 15; pymf/greedy.py for dense data, Civril and Magdon-Ismail: W = the num_bases data columns that best reproduce
 * the leading singular subspace, chosen one after the other; H = pinv(W) data).  Dense resident data, one rank, num_bases <= 64,
 * min(rows, cols) <= 2432 -- PMF_EINVAL otherwise.  The data are never rewritten: the reference's normalise-and-deflate loop is
 * restated on the read-only data (pmf_greedy.h).
 *   pmf_update_w     GREEDY.update_w (greedy.py:88-170): the eigenpairs of the float64 Gram matrix on the short side, then
 *                    rows <= cols: num_bases rounds of one pass over V (k_greedy_pass) and one float64 step (k_greedy_step)
 *                    enqueued back to back; rows > cols: all rounds in Gram space (k_greedy_gram).  Then W = V[:, select];
 *                    needs V only.  pmf_sivm_get_select reads the selection.  Two runs give the same bits.
 *   pmf_update_h     GREEDY.update_h (greedy.py:82-86): H = pinv(W) V, pinv(W) = (W^T W)^+ W^T in float64 with svd.py's cut
 *                    (eigenvalues <= 1e-8 dropped), rounded once, the product on the fp32 MFMA; needs V and W.
 *   pmf_factorize    NMF.factorize's loop; the steps repeat their result, so the convergence test stops it at the third iteration.
 *   pmf_frobenius    the direct residual.
 * A column whose residual against the columns chosen so far is at rounding level (norm^2 <= 512 unit roundoffs of its norm^2)
 * scores 0; when every column does, the lowest index not yet chosen is taken.
 * pmf_greedy_select: the selection alone -- nsel <= 64 indices in selection order -- among the columns of V (transposed = 0) or
 * among its rows (transposed = 1: GREEDY on the transposed view, what GREEDYCUR's row selection is), on a GREEDY or a CUR / CMD
 * context.  Both calls share the Gram matrix and its eigenpairs, formed once per V.
 * On CSR data (pmf_set_v_csr_f32 on a GREEDY context; path "greedy_csr"; min(rows, cols) padded to 64 at most 1024) the data stay
 * sparse through all rounds (the reference's sparse branch, greedy.py:115-141, holds a dense matrix from the second round on).
 * The Gram matrix of the short side comes from the stored entries in exact fixed point (k_csr_gram); solver, cut and order are
 * those of dense data.  Where the candidates lie on the long side, a round is k_greedy_csr_pass -- a wave per CSR line of the
 * image whose lines are the candidates (both images are resident: pmf_greedy_select with transposed = 1 needs no copy), float64
 * sums of exact products against the staged operand, the same score and guard, one partial per workgroup -- and
 * k_greedy_step_csr, k_greedy_step with the chosen column read from its CSR line.  Otherwise k_greedy_gram runs as on dense data.
 * W = V[:, select] is scattered from the image of V^T (k_greedy_csr_gather).  pmf_update_h: H^T = V^T pinv(W)^T in float64, one
 * k_csr_proj_f64 pass; H stays float64 on the device and is read through pmf_get_h_f64 / pmf_get_h_f32.  pmf_frobenius and the
 * error of pmf_factorize: the float64 identity ||data||^2 - 2 <W^T data, H> + <W^T W, H H^T>, clamped at 0 before the root.  Two
 * runs give the same bits.  pmf_profile_enable times k_greedy_csr_pass. */
int pmf_greedy_select(pmf_ctx* ctx, int32_t transposed, int32_t nsel, int32_t* select);

/* Device time (ms, HIP events on the library's stream) of the last pmf_factorize loop. */
int pmf_last_loop_ms(pmf_ctx* ctx, double* ms);

/*
 * Per-kernel timing for bench.py's roofline: when enabled, every launch of the
 * dominant kernel of the current algo is bracketed by HIP events on the
 * library's stream.  pmf_kernel_stats returns the kernel's name, launch count
 * and mean duration since the last reset.
 */
int pmf_profile_enable(pmf_ctx* ctx, int32_t on);
int pmf_kernel_stats(pmf_ctx* ctx, const char** name, int64_t* launches, double* mean_ms,
                     double* flops_per_launch, double* bytes_per_launch);

/* Host-only helper of the boundary (touches no device): an order-dependent 128-bit digest of `nbytes`
 * bytes of caller memory, out2[0..1].  The reference always computes from the CURRENT contents of
 * self.data / self.W / self.H (nmf.py:122-132); a host class that keeps device copies uses this to notice
 * in-place edits (permutations included) and re-upload.  Multi-threaded, memory speed. */
int pmf_host_checksum(const void* data, uint64_t nbytes, uint64_t* out2);

/* Tuning knobs (results agree to rounding whatever they say).  The tag of each says why it exists: [transport] how the
 * cross-rank sums travel, [measurement] a timing or counting hook, [size override] forces a choice the library makes from
 * the problem's size, [test reference] selects the kernel that the tests compare the default one against.  Known names:
 *   "oneshot_allreduce" [transport] 1 / 0: small cross-rank sums on the one-shot IPC all-reduce (after pmf_ipc_import) or
 *                on the context's other transport.
 *   "profile_every" [measurement] N >= 1 (default 1): with pmf_profile_enable only every N-th launch of the dominant kernel
 *                (and of the per-iteration collective) carries HIP events -- a timed launch costs the loop about 5 us.
 *   "fold_exchange" [transport] 1 (default) / 0: inside pmf_factorize's one-pass NMF / BNMF loop the per-iteration sum of
 *                (W^T V | W^T W) rides on the launches around it -- the slab reduce pushes this rank's partial tiles into
 *                every peer's receive area, the H-step launch waits for the peers' flags in its prologue and adds the N
 *                partials in rank order -- instead of a k_ipc_allreduce launch of its own.  Bit-identical either way.
 *   "snmf_w_pipe" [test reference] snmf_gram = 2 on CSR data: the W = V M write of iteration i runs on a stream of its own
 *                beside the k x n sized kernels of iteration i + 1 (they never read W; M is double buffered); the value is
 *                the number of workgroup slots the write launch leaves free so that those kernels can be placed while it
 *                runs (default 32); 0: everything in stream order.  Bit-identical results.
 *   "nnqp_count" [measurement] 1: the W half steps of NMFALS / NMFNNLS run the COUNTING instantiation of the
 *                sixteen-lanes-per-problem kernel (pmf_nnqp_counters; it costs the kernel 8 %); 0 (default): no counters.
 *   "snmf_gram"  [size override] SNMF loops with both updates on iterate in Gram space -- P = M^T (V^T V), S = P M on
 *                k x n sized data, W materialised once after the last iteration -- instead of one pass
 *                over V per iteration: -1 automatic (default: CSR data always, dense data from about
 *                n / 2k iterations on), 0 never, 1 whenever the shape allows (n <= 1024), 2 as 1 but W = V M is
 *                written in EVERY iteration (what the reference's update_w does; same results).
 *   "nnqp_quad"  [size override] NMFALS / NMFNNLS with num_bases <= 64 and a well-conditioned Hessian: the half step's QPs
 *                on the sixteen-lanes-per-problem kernel (block principal pivoting on the smaller of HA[P,P] /
 *                inv(HA)[N,N]): 1 (default) from 16 384 problems per half step on, 2 always, 0 never (the
 *                lane-per-variable kernel).  Same minimisers (they are unique).
 *   "nndsvd_topk" [size override] pmf_nndsvd_init's eigen-solver: -1 (default) full Jacobi up to 1024 columns and the
 *                top-k subspace iteration beyond, 1 / 0 force one of them where both apply (top-k needs num_bases + 16 <= n,
 *                Jacobi n <= 4096).  Same W, H to ~1e-8 (well inside the float32 accuracy of the Gram matrix).
 *   "colgemm_stream" [test reference] 1 (default): the W^T V | W^T W partials of the two-pass path on k_colgemm_stream (V
 *                fragments straight into registers, requests interleaved with the MFMAs, W rows through LDS once per
 *                workgroup) where it applies (16 < num_bases <= 64; blocks of 128 bases); 0: k_colgemm.  Bit-identical.
 *   "rowgemm_stream" [test reference] 1 (default): plain products with a long contraction (V H^T of NMFALS / SNMF,
 *                W = V M^T) on k_rowgemm_stream (A fragments straight into registers, requests interleaved with the
 *                MFMAs); 0: on k_rowgemm.  Bit-identical results (same order of summation).
 *   "nnqp_frame16" [test reference] 1 (default): the sixteen-lanes-per-problem kernel first on a 16-slot frame (settled
 *                active sets factorise systems of about 8 unknowns: twelve waves around one LDS image of HA and inv(HA),
 *                168 registers -- three waves per SIMD instead of two), problems that outgrow it on the 32-slot frame
 *                behind; 0: the 32-slot frame for all.  Bit-identical results.
 *   "nnqp_wave"  [test reference] 1 (default): NMFALS / NMFNNLS sub-problems at 64 < num_bases <= 128 on k_nnqp_wave (one
 *                wave per problem, block principal pivoting on the smaller of HA[P,P] / inv(HA)[N,N], LDL^T in
 *                registers); 0: k_nnqp_big (one variable at a time, the inverse image in global memory).  Same KKT point,
 *                float32 results equal to rounding.
 *   "force_tiled" [test reference] 1: every path of this context takes the any-shape two-pass kernels (k_rowgemm /
 *                k_colgemm) even where a one-pass kernel covers the shape; 0 gives the one-pass kernels back.  For tests
 *                and measurements of the any-shape kernels on the bench shapes.
 * SNMF with num_bases <= 128 always keeps H in FLOAT64 on the device (the reference's H is float64, pymf/nmf.py:120, and
 * W = V H^T inv(H H^T) amplifies its rounding by sigma_max / sigma_min of H): G = H H^T, M^T = inv(G) H and the H step
 * (snmf.py:72-91, on the float64 MFMA) read and write that copy; the float32 H is its rounding. */
int pmf_set_option(pmf_ctx* ctx, const char* name, int64_t value);

/* Host transport for the cross-rank sums, for set-ups in which the ranks cannot form an RCCL communicator
 * (plumbing checks with several ranks sharing one GPU; ranks without a common fabric).  Contexts created
 * with nranks == 1 and no nccl_id only.  fn(user, buf, count, is_f64) must replace the `count` floats
 * (is_f64 = 0) or doubles (1) at host pointer `buf` by their sum over all ranks and return 0; every
 * rank's library calls it at the same points in the same order (where the RCCL build runs
 * ncclAllReduce).  Each call is a blocking device -> host -> device round trip: not a fast path. */
typedef int (*pmf_host_allreduce_fn)(void* user, void* buf, int64_t count, int32_t is_f64);
int pmf_set_host_allreduce(pmf_ctx* ctx, pmf_host_allreduce_fn fn, void* user);

/* One-shot all-reduce for the small per-iteration sums (the reduction over m of pymf/nmf.py:124-125 is what
 * the row sharding splits): every rank owns a receive area that all peers map through HIP IPC; ONE kernel per rank writes
 * its partial of (W^T V | W^T W) into every peer's area, raises a flag there, waits for the peers' flags and adds the N
 * partials in rank order -- bit-identical sums on all ranks, no ring / tree hops.  Payloads up to 256 KiB take it; larger
 * ones (the n x n float64 V^T V of the Gram-space SNMF loop, NNDSVD's Gram matrix) stay on RCCL / the host transport.
 *   pmf_ipc_export(ctx, rank, nranks, handle_out)   allocate + export this rank's area (sized for nranks; also the self-test's
 *                                                   buffers, so that nothing is allocated between the test's collectives)
 *   (hand every rank's handle to every rank by any means, in rank order)
 *   pmf_ipc_import(ctx, handles, nranks)            map the peers' areas (the SAME nranks; all or nothing: a failing
 *                                                   hipIpcOpenMemHandle closes what was opened); from here on small sums take
 *                                                   the one-shot path -- inside pmf_factorize's one-pass loop folded into the
 *                                                   slab-reduce and H-step launches (option "fold_exchange")
 * 2 <= nranks <= 8, one node (ranks on different GPUs of one xGMI hive, or -- for plumbing checks -- sharing a GPU).
 * pmf_collective_name: which transports this context's cross-rank sums use and how often each ran. */
#define PMF_IPC_HANDLE_BYTES 64
int pmf_ipc_export(pmf_ctx* ctx, int32_t rank, int32_t nranks, void* handle_out);
int pmf_ipc_import(pmf_ctx* ctx, const void* handles, int32_t nranks);
/* The one-shot path against the context's other transport (RCCL / host) on rank- and round-dependent payloads, `rounds`
 * times (both slots get reused; odd rounds in the split producer / consumer form the loop uses): *ok = 1 iff all rounds agreed
 * and no wait ran out (2 s per wait).  Every rank calls it at the same
 * point; the caller combines the verdicts and switches the path off on ALL ranks if any disagreed
 * (pmf_set_option(ctx, "oneshot_allreduce", 0)). */
int pmf_ipc_selftest(pmf_ctx* ctx, int32_t rounds, int32_t* ok);
const char* pmf_collective_name(pmf_ctx* ctx);

/* Forget everything derived from V (||V||^2, cached partial sums): for streamed `data` that the caller
 * rebound or edited between calls. */
int pmf_invalidate_v(pmf_ctx* ctx);

/* A W step that can fail -- SNMF: np.linalg.inv raises on a singular H H^T BEFORE W is rebound (snmf.py:69-70) --
 * must leave the previous W behind.  The host class keeps W on the device between calls, so before such a step it
 * asks for a device-side copy (pmf_snapshot_w: one device-to-device copy, W materialised first if it was implicit) and
 * puts it back when the step raised (pmf_restore_w).  No host traffic either way. */
int pmf_snapshot_w(pmf_ctx* ctx);
int pmf_restore_w(pmf_ctx* ctx);
/* The same for H (k x n: small), together with what the device derived from it (NMF / BNMF: the Gram matrix H H^T as the last
 * H step left it, so that a restored H continues with the same bits).  With pmf_snapshot_w / pmf_restore_w: the pair of factors
 * a loop started from, for a caller that finds out DURING the loop that it has to start again (pmf_abort). */
int pmf_snapshot_h(pmf_ctx* ctx);
int pmf_restore_h(pmf_ctx* ctx);

/* With pmf_profile_enable the per-iteration collective -- the sum of (W^T V | W^T W) over the ranks, what the row sharding of
 * pymf/nmf.py:124-125 costs -- is bracketed by HIP events as well: mean duration (ms) and count since the last enable. */
int pmf_collective_ms(pmf_ctx* ctx, double* mean_ms, int64_t* count);

/* The flops one launch of that kernel really executes (pmf_kernel_stats reports SURVEY's algorithmic
 * count): W^T W is symmetric (upper triangle only) and SNMF's W step is reassociated. */
int pmf_kernel_exec_flops(pmf_ctx* ctx, double* executed_flops_per_launch);

/* The individual launch durations behind pmf_kernel_stats' mean, in launch order: out_ms[0..min(cap,*count))
 * (ms, HIP events on the library's stream); *count = launches recorded since the last pmf_profile_enable. */
int pmf_kernel_launch_ms(pmf_ctx* ctx, double* out_ms, int64_t cap, int64_t* count);

/* NMFALS / NMFNNLS on the sixteen-lanes-per-problem kernel (pymf/nmfals.py:85-97, the row QPs of update_w): running totals
 * since the last reset, counted on the device by the kernel itself -- out8[0..3] for the 16-slot frame, out8[4..7] for the
 * 32-slot frame: wave tasks (4 problems each), passes (one solve per problem each), the sum over the passes of the largest
 * system among the wave's four problems (the size the frame-padded elimination runs over), problems solved on that frame.
 * bench.py's roofline block is built from them (live counts instead of recorded constants). */
int pmf_nnqp_counters(pmf_ctx* ctx, int64_t* out8, int32_t reset);

int pmf_synchronize(pmf_ctx* ctx);
/* The ONE entry point that may be called from a second host thread while pmf_factorize runs on the context: on = 1 makes the
 * running (or the next) pmf_factorize return at its next iteration / chunk boundary with *iters_done = what it completed;
 * on = 0 clears the request.  The host class runs its digest of `data` (the reference re-reads self.data[:,:] in every hook,
 * nmf.py:123,129) BESIDE the device loop and, should the bytes have changed since the upload, stops the loop, puts W / H back
 * (pmf_restore_w, pmf_restore_h), uploads and starts again. */
int pmf_abort(pmf_ctx* ctx, int32_t on);

/* Introspection used by tests: which code path update_w/update_h take for this shape.
 * Returns a static string such as "fused_k64_n256" or "tiled". */
const char* pmf_path_name(const pmf_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* PYMF_HIP_H */
