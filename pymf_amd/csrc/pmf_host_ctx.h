// pmf_host_ctx.h -- the context (pmf_ctx), error plumbing (fail / HIPCHK / PMFCHK), device memory (dalloc / dfree / dgrow),
// the event brackets of the profiled launch site, need() and the invalidation functions (v_replaced ... sums_dropped).
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

constexpr int PMF_HGRAM_MAX_WGS = 64;

std::string g_create_error;

// Launch sites that can be bracketed by HIP events (pmf_profile_enable): ONE of them, the dominant
// m-sized kernel of the path the context takes, is recorded at a time (choose_stat_site).
enum { SITE_NONE = 0, SITE_FUSED, SITE_ROWGEMM_W, SITE_NNQP_W, SITE_MATERIALIZE, SITE_CSR_PASS, SITE_CLUSTER, SITE_SIVM, SITE_SIVM_ROWS, SITE_AA, SITE_SVD, SITE_CUR, SITE_GREEDY, SITE_CUR_LEV, SITE_CUR_SQNORMS, SITE_LAESA, SITE_GMAP, SITE_SGREEDY, SITE_VQ, SITE_VQ_ARGMIN, SITE_GATHER };

struct KernelStat {
  std::string name = "none";
  int site = SITE_NONE;
  double flops = 0.0, bytes = 0.0, exec_flops = 0.0;
  std::vector<hipEvent_t> ev;   // pairs
  size_t used = 0;              // events recorded since reset
  int every = 1;                // pmf_set_option("profile_every", N): only every N-th launch of the site carries events -- a pair costs
                                // the loop ~5 us (the queue processes two more packets and the dispatch's completion signal): 8 % of a
                                // 60 us iteration when every launch is timed (tools/loop_probe.py, profiles/r05_experiments.md)
  int64_t seen = 0;             // launches of the site since reset
  bool open = false;            // stat_begin recorded, stat_end to follow
};

}  // namespace

struct pmf_ctx {
  int algo = 0;
  int64_t m = 0, n = 0;
  int k = 0, device = 0, rank = 0, nranks = 1;
  int nb = 1;                   // > 1: num_bases > 128 (NMF): KP = 128 nb, bases handled in blocks of 128
  std::vector<void*> owned;     // every device buffer of the context (dalloc / dalloc_raw): what dfree and pmf_ctx_destroy release
  float* dW2 = nullptr;         // ... Den = W (H H^T), [mp][KP] (dW1 holds Num = V H^T)
  float* dWideT = nullptr;      // chunk result of a product over more than PMF_WIDE_K columns
  int64_t wide_cap = 0;
  float *dWideN = nullptr, *dWideD = nullptr;   // ... Num and Den of the W rules there (wide_update_w_rows)
  int64_t wide_nd_cap = 0;
  int64_t mp = 0;
  int np = 0, KP = 0, NT = 0;
  hipStream_t stream = nullptr;
  ncclComm_t comm = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float *dV = nullptr, *dW = nullptr, *dH = nullptr, *dG = nullptr, *dPS = nullptr;
  float *dSlab = nullptr, *dW1 = nullptr, *dGinvT = nullptr;
  float* dMT = nullptr;         // SNMF: M^T = inv(H H^T) H, [KP][np] (k_snmf_mt)
  double* dGinvD = nullptr;     // SNMF: inv(H H^T) in float64, [KP][KP]
  // Gram-space SNMF loop (snmf_gram_iteration): C = V^T V over all ranks' rows, and the float64 M^T, P
  double *dC = nullptr, *dMTd = nullptr, *dPd = nullptr;
  // SNMF (num_bases <= 128): H in float64 on the device (pmf_inv.h, round 6) -- dH is its float32 rounding.  hd_synced: k_hd_sync
  // has compared the two in THIS API call (need() clears it); ps_f64: (P | S) of the Gram-space iteration at hand are in dPd / dSd
  double *dHd = nullptr, *dSd = nullptr, *dHdSnap = nullptr;
  bool hd_synced = false, hd_force = false, ps_f64 = false;   // hd_force: H was replaced through a float32 entry point.  hd_synced, hd_force <- H
  bool psd_fresh = false;      // dPd / dSd are the float64 (P | S) of the CURRENT W (set by a Gram-space iteration, for the error behind it; every API entry clears it: need())
  double* dCslabs = nullptr;    // k_csr_gram: per-workgroup images of C's upper triangle (two 64-bit fixed-point limbs per entry)
  unsigned* dVmaxBits = nullptr; // ... and the bit pattern of the largest |v| (the limbs' grids)
  bool c_valid = false;         // dC holds the all-rank V^T V of the current V.  <- V, the transport of the cross-rank sums
  int opt_snmf_gram = -1;       // pmf_set_option("snmf_gram"): -1 auto, 0 never, 1 whenever possible, 2 = 1 + W written in every iteration
  bool w_implicit = false;      // the loop ran in Gram space: dW is stale, W = V M with the M at hand (materialize_w).  <- W (CNMF: set by a new G)
  // snmf_gram = 2 on CSR data: W = V M of iteration i is written on a stream of its own BESIDE the k x n sized kernels of
  // iteration i + 1 (they never read W); M is double buffered (dW1, dW1 + np KP) and the write launch leaves a few
  // workgroup slots free so that the small kernels can be placed while it runs (w_pipe_* below, materialize_w)
  hipStream_t w_stream = nullptr;
  hipEvent_t ev_mt[2] = {nullptr, nullptr}, ev_w[2] = {nullptr, nullptr};
  bool ev_w_pending[2] = {false, false};
  int64_t w_pipe_it = 0;        // writes enqueued so far: buffer parity
  int opt_w_pipe = 32;          // pmf_set_option("snmf_w_pipe"): workgroup slots the write launch leaves free; 0 = in stream order
  float* dD = nullptr;          // RNMF: D = S - V (rnmf.py:102,111), [mp][np]
  bool s_valid = false;         // RNMF: D has been formed (update_s ran)
  double rnmf_err2 = -1.0;      // RNMF: sum((V - W H)^2) from the last update_s (all ranks)
  double *dGd = nullptr, *dPart = nullptr, *dScal = nullptr;
  double* dGramPart = nullptr;  // k_gram_splitk: per-slice partial Gram matrices, [8][KP][KP]
  unsigned* dGramTickets = nullptr;   // k_gram_splitk: one per tile
  float* dGpart = nullptr;      // k_nmf_h_gram: per-workgroup partial G, [PMF_HGRAM_MAX_WGS][KP][KP]
  float* dHsnap = nullptr;      // pmf_snapshot_h: H, then G, then the partial Gs
  bool hsnap_valid = false, hsnap_g_valid = false;
  int hsnap_g_parts = 0;
  double* dT1part = nullptr;    // ... and partial <P, H_new>
  unsigned* dTicket = nullptr;  // ... arrival counter (the kernel resets it)
  // free-running pmf_factorize loop: device-side error history and stop flag
  double* dFerr = nullptr; int64_t ferr_cap = 0;
  int* dStop = nullptr;         // [0] 0 run / 1 converged / 2 identity cancels, [1] iteration
  int* dWarm = nullptr;         // k_nnqp: warm start allowed (k_spd_unique)
  const int* stop_arg = nullptr;   // what the loop kernels get: dStop while free-running, else NULL
  // free-running loop: the error / convergence test of iteration conv_iter (>= 0) is still to be evaluated, from
  // conv_ntt pairs of trace terms at conv_tt; the next one-pass launch does it in its prologue (FusedCtl)
  int conv_iter = -1, conv_ntt = 0;
  const double* conv_tt = nullptr;
  double conv_eps = 0.0;
  // CSR V (SNMF sparse path)
  int64_t* dIndptr = nullptr; int32_t* dIndices = nullptr; float* dVals = nullptr; int64_t nnz = 0;
  bool v_csr = false;
  bool v_csc = false;           // SIVM / LAESA on CSC data (pmf_set_v_csc_f32): the three arrays above hold the COLUMNS of V (indptr [np + 1]), dV is released
  int opt_sivm_csc_team = 0;    // pmf_set_option("sivm_csc_team"): 0 by the mean column length, or 4, 16, 64 lanes per column in k_sivm_csc_pass
  bool csr_dense = false;       // CSR data with num_bases > 128: a dense image in dV serves the data paths (no CSR kernel at that width)
  // NMF on CSR data (pmf_nmf_csr.h, pmf_host_nmf_csr.h): the CSR arrays of V^T (built on the host by pmf_set_v_csr_f32), the working
  // copy H^T [np][KP], S = W^T W [KP][KP] (the G of the H step), the workgroups' slabs of k_nmf_sp_step
  int64_t* dTIndptr = nullptr; int32_t* dTIndices = nullptr; float* dTVals = nullptr;
  float *dHT = nullptr, *dSw = nullptr, *dSpSlab = nullptr;
  int sp_wgs_cap = 0;           // slabs dSpSlab holds
  bool ht_valid = false;        // dHT = dH^T.  <- H
  bool ht_newer = false;        // an H step wrote dHT and dH has not followed yet (nmf_csr_sync_h).  <- H
  bool sw_valid = false;        // dSw = W^T W of the current W.  <- W
  std::string path_dense;       // pmf_path_name of the context with dense data (CSR data on an NMF context: "nmf_csr_gather")
  int* dSing = nullptr;         // SNMF: raised by the inverse kernels when H H^T has a zero pivot (check_singular)
  double* dQp = nullptr;        // k_nnqp_big (NMFALS, num_bases > 64): per-workgroup inverse images
  double* dBinv = nullptr;      // k_nnqp_quad: B = inv(HA), [KP][KP] float64
  int* dDefer = nullptr;        // k_nnqp_quad<16>: problems left to the 32-slot frame
  int64_t defer_cap = 0;
  int* dNbig = nullptr;         // [2 sites][3 + 2]: rotating counters of k_nnqp_quad (QuadCtl: nbig x 3, dcount x 2)
  int64_t quad_calls[2] = {0, 0};
  unsigned long long* dQstat = nullptr;   // k_nnqp_quad, W half steps: [2 frames][4] running totals (pmf_nnqp_counters)
  double* dY0 = nullptr;        // k_nnqp_wave: inv(HA) f of every problem of a half step
  int64_t y0_cap = 0;
  int opt_nnqp_wave = 1;        // pmf_set_option("nnqp_wave"): 64 < num_bases <= 128 on the wave-per-problem block-pivoting kernel
  int opt_nnqp_frame16 = 1;     // pmf_set_option("nnqp_frame16"): the 16-slot frame first (three waves per SIMD)
  int opt_nnqp_count = 0;       // pmf_set_option("nnqp_count"): the counting instantiations of k_nnqp_quad (pmf_nnqp_counters)
  void* dStage = nullptr;       // staging area of the host <-> device transport (upload_rows / download_rows)
  size_t stage_cap = 0;
  float* dWsnap = nullptr;      // pmf_snapshot_w: the W before a step that may fail
  bool wsnap_valid = false;
  int opt_nndsvd_topk = -1;     // pmf_set_option("nndsvd_topk"): -1 by size, 1 the filtered subspace iteration, 0 full Jacobi
  int nndsvd_products = 0;      // products with the Gram matrix the last top-k solve took
  int opt_colgemm_stream = 1;   // pmf_set_option("colgemm_stream"): W^T V partials on k_colgemm_stream where it applies
  int opt_resid_resident = 1;   // residual pass with H resident in LDS (k_resid_res) where it fits
  int resid_parts = 0;          // float64 partials the last residual pass left in dPart
  int64_t dpart_cap = 0;        // doubles dPart holds
  int opt_rowgemm_stream = 1;   // pmf_set_option("rowgemm_stream"): plain products with a long contraction on k_rowgemm_stream
  int opt_nnqp_quad = 1;        // pmf_set_option("nnqp_quad"): num_bases <= 64 on the sixteen-lanes-per-problem kernel
  double *dInvA = nullptr, *dInvB = nullptr;   // k_inverse_spd_big: the two images of the elimination, [KP][KP]
  int nchunks = 0, rows_per_chunk = 0;
  int fused_wgs = 0;            // >0: fused one-pass kernel available for this shape
  int fused_wgs_hidden = 0;     // pmf_set_option("force_tiled", 1) parks fused_wgs / fused8 here: every path then takes the
  bool fused8_hidden = false;   // any-shape two-pass kernels (k_rowgemm / k_colgemm) -- test and measurement aid
  std::string path_hidden;
  bool fused8 = false;          // ... and it is the cooperative form (pmf_coop.h: 64 < k <= 128, or k <= 64 with n > 256)
  int coop_bt = 0, coop_rb = 0; // its base tiles per wave / row blocks per tile
  bool have_v = false, have_w = false, have_h = false, g_valid = false;   // g_valid: dG = H H^T.  g_valid, g_parts <- H
  int g_parts = 0;              // > 0 (with g_valid): G = sum of that many partials in dGpart, dG is stale
  int trace_parts = 0;          // > 0 (with trace_ready): the trace terms are that many pairs in dT1part
  bool gram_partial_ok = false; // pmf_factorize: the next consumer of G is the fused kernel
  bool want_hess = false, gd_is_s = false;   // NMFALS H half step: the reduce writes dGd = W^T W itself (reduce_slabs)
  bool ps_valid = false;        // dPS = (W^T V | W^T W) of the CURRENT W, summed over all ranks.  <- V (RNMF: D), W, the transport
  bool num_valid = false;       // dW1 holds Num = V H^T of the current V, H (fixed-H loops, NMF).  <- V, H; W too: dW1 is also the W steps' scratch
  bool fixed_h_loop = false;    // pmf_factorize running compute_w without compute_h for > 1 iteration
  bool want_trace = false;      // pmf_factorize with PMF_COMPUTE_ERR: let the H-step kernel emit the trace terms
  bool trace_ready = false;     // dScal[2..3] already hold <P,H>, <S,HH^T> for the current W, H.  <- V, W, H, the transport (read with ps_valid only)
  bool vnorm_valid = false;     // vnorm2 is current.  <- V, the transport
  bool vnorm_local_valid = false;   // dScal[6] = sum(V^2) over this rank's rows (formed behind the upload).  <- V
  double vnorm2 = 0.0;          // ||V||_F^2 over all ranks
  // CNMF (pmf_cnmf.h; num_bases <= 128, H in dHd / dH): G^T [KP][np], the split products (neg(C) G)^T, (pos(C) G)^T and
  // H neg(C), H pos(C) (the latter two also hold Z^T, (C Z)^T of the k-means initialisation), L_A = A^T G, L_B = B^T G,
  // the error terms; k-means: assignment, member counts, squared distances, z^T C z, the selected samples
  double *dGT = nullptr, *dCnA = nullptr, *dCnB = nullptr, *dCnHn = nullptr, *dCnHp = nullptr, *dCnLA = nullptr, *dCnLB = nullptr,
         *dCnTT = nullptr, *dKmDmin = nullptr, *dKmZcz = nullptr;
  int *dKmAsg = nullptr, *dKmCnt = nullptr, *dKmSel = nullptr;
  bool have_g = false;          // G set (pmf_set_g_f64 / pmf_cnmf_init)
  bool cn_ab_valid = false;     // dCnA / dCnB belong to the current G and C.  <- G, V (through c_valid: cnmf_ensure_c)
  bool cn_l_valid = false;      // dCnLA / dCnLB belong to the current G and C.  <- G, V (as above)
  bool cn_user_w = false;       // W was uploaded by the caller (not V G): the error is the direct residual with it.  <- W from the caller
  double cn_trc = 0.0;          // tr(C) of the current C
  // Kmeans / Cmeans (pmf_cluster.h): per-workgroup slabs of V H^T, of the denominators and of the error, ||w_j - mu||^2, their
  // totals ([KP] denominators, then sum_c min_j d^2 and sum_c ||v_c - mu||^2), the assignment, mu = the row means of V
  float *dClNum = nullptr, *dClMu = nullptr;
  double *dClDen = nullptr, *dClErr = nullptr, *dClWn = nullptr, *dClTot = nullptr;
  int* dClAsg = nullptr;
  int cl_wgs = 0, cl_ppw = 0;   // workgroups of k_cluster_pass, 64-column panels each owns
  bool cl_have_asg = false;     // dClAsg holds an assignment (Kmeans: an H step ran, or pmf_cluster_set_assigned)
  bool cl_sums_valid = false;   // the slabs belong to the current V and assignment (Kmeans) / H (Cmeans).  <- V, H (Cmeans), the assignment
  bool cl_mu_valid = false;     // dClMu holds the row means of the current V.  <- V
  bool cl_err_valid = false;    // dClTot[KP] = ||V - W H||^2 of the current V, W, H (Kmeans, right behind its H step).  <- V, W, H
  // Kmeans / Cmeans on CSR data (pmf_cluster_csr.h, pmf_host_cluster_csr.h): v_csr with both CSR images resident and no dV, as on a
  // CUR / CMD context.  H lives as H^T [np][cc_ld] float64 (dH is not used while CSR data is resident); |v|^2 of the rows [mp] and
  // behind them of the samples [np]; the chunks of the data rows (cc_chunks of them: the first chunk of every row [mp + 1], the row
  // of every chunk) with their partial sums [cc_chunks][cc_ld]; the partials of the denominators and of the error per workgroup
  // of the H step, their totals [cc_ld + 2], |w_c|^2 [cc_ld].  dClAsg and the cl_* flags are shared with the dense path.
  double *dCcHT = nullptr, *dCcSq = nullptr, *dCcPart = nullptr, *dCcDen = nullptr, *dCcErr = nullptr, *dCcTot = nullptr, *dCcWn = nullptr;
  int *dCcChunkOff = nullptr, *dCcChunkRow = nullptr;
  int cc_ld = 0, cc_chunks = 0, cc_wgs = 0, cc_lpw = 0;
  // SIVM (pmf_sivm.h): the recurrence's state ([3][np] float64), the two partials arrays of the argmax (scores, indices), select,
  // (maxd, a); H step: the right-hand sides f + lambda [KP][np], the brackets [6][np], their sides, unfinished columns per round
  double *dSvState = nullptr, *dSvPart = nullptr, *dSvScal = nullptr, *dSvLam = nullptr;
  int *dSvPartIdx = nullptr, *dSvSel = nullptr, *dSvSide = nullptr, *dSvUnf = nullptr;
  float* dSvF = nullptr;
  int sv_wgs = 0, sv_ppw = 0;   // AA: workgroups of k_aa_price, 64-column panels each owns (k_sivm_pass takes its partition per call)
  int sv_metric = 0;            // pmf_set_option("sivm_metric"): 0 l2, 1 l1, 2 cosine
  int sv_init = 0;              // pmf_set_option("sivm_init"): 0 fastmap, 1 origin
  int sv_rule = 0;              // pmf_set_option("sivm_rule"): 0 SIVM, 1 LAESA, 2 GMAP (pmf_colsel.h) -- what pmf_update_w selects by
  int sv_gmap_method = 0;       // pmf_set_option("gmap_method"): 0 pca, 1 aa, 2 nmf
  bool sv_have_select = false;  // dSvSel holds the selection of a W step
  // SIVM_SGREEDY (pmf_sgreedy.h): the squared distances to the selected columns ([64][np] float32), inv(CM_S) [64][64], the
  // rounds' volumes and scale_t; allocated by the first selection under the option
  float* dSgTab = nullptr;
  double *dSgM = nullptr, *dSgVol = nullptr;
  int sv_sgreedy = 0;           // pmf_set_option("sivm_sgreedy"): pmf_update_w selects by the exact simplex volume (sv_rule stays 0)
  bool sg_have_vol = false;     // dSgVol holds the volumes of a W step
  // SIVM_GSAT (pmf_gsat.h): the vertices as rows ([k][m] float32); float64: the distance table [64][64], the last probe's distances
  // [64], V; per launch the probes' volumes [256] and distances [256][64]; allocated by the first pmf_gsat_start.  On the host
  // V and the reference's _v since the start ([V at the first swap, the accepted volumes ...])
  float* dGsW = nullptr;
  double *dGsTab = nullptr, *dGsProbe = nullptr;
  int* dGsCtl = nullptr;        // [0] the accepted position of a launch, [1] accepted volumes of the call
  int sv_gsat = 0;              // pmf_set_option("sivm_gsat"): the W step is pmf_gsat_walk / pmf_gsat_probe_vec, pmf_update_w refuses
  bool gs_started = false;      // the walk's state belongs to the context's W.  <- W from the caller
  double gs_V = 0.0;
  std::vector<double> gs_log;
  int opt_profile_sivm_rows = 0;   // pmf_set_option("profile_sivm_rows"): pmf_profile_enable times the rounds of the long-sample pass (SITE_SIVM_ROWS)
  // AA (pmf_aa.h): W_hat, the points X and residuals R ([mp][KP]); the two partials arrays of the pricing pass ([2][wgs][KP]); per
  // base the corral's Gram matrix, data columns and weights by slot, the finished flag; unfinished bases per round; the
  // inverse's verdict (zero pivot, pivots above 1e-8), inv(H H^T), beta [k][n]
  float *dAaWhat = nullptr, *dAaX = nullptr, *dAaR = nullptr, *dAaScore = nullptr;
  int *dAaIdx = nullptr, *dAaSlot = nullptr, *dAaFin = nullptr, *dAaUnf = nullptr, *dAaFlag = nullptr;
  double *dAaGram = nullptr, *dAaLam = nullptr, *dAaGinv = nullptr, *dAaBeta = nullptr;
  int aa_rounds = 0;            // rounds the last W step took
  bool aa_have_beta = false;    // dAaBeta holds the weights of a W step
  // CHNMF (pmf_chnmf.h, on an AA context): R [16][mp] and proj = R V [16][np] in float64; per pair the partials of the extremes
  // ([wgs][128] scores and indices, [wgs] largest magnitudes), the polygon's edges, the filter's flags [np] and counts [wgs], the
  // survivors [4096]; the survivor counts of all pairs (and, last, the size of the union); the union's mask [np] and indices [np]
  double *dChR = nullptr, *dChProj = nullptr, *dChPscore = nullptr, *dChPmax = nullptr, *dChEdges = nullptr;
  int *dChPidx = nullptr, *dChCounts = nullptr, *dChSurv = nullptr, *dChNsurv = nullptr, *dChIdx = nullptr;
  unsigned char *dChKeep = nullptr, *dChMask = nullptr;
  int ch_cap = 0, ch_max_wgs = 0;   // pmf_chnmf_set_limits: survivors k_hull_chain takes / workgroups of the sweeps (0: the build's)
  int ch_routes[3] = {0, 0, 0};     // pairs of the last pmf_chnmf_hull by route: 32 directions, 128 directions, host
  // SVD / PCA (pmf_svd.h): the kept eigenvectors in descending order ([KP][mp] or, rows > cols, [KP][np]; float64), the singular
  // values [KP], the projected side in float32 (V [KP][np] or, rows > cols, U [mp][KP])
  double *dSvdE = nullptr, *dSvdS = nullptr;
  float* dSvdP = nullptr;
  int svd_rank = 0;             // eigenvalues above svd.py's 1e-8 cut
  bool svd_left = false;        // rows > cols: svd.py's _left_svd
  bool svd_valid = false;       // dSvdE / dSvdS / dSvdP belong to the current V.  <- V
  int pca_bases = 0;            // pmf_set_option("pca_num_bases"): columns of U that PCA's W step takes, 0 = all
  // SVD / PCA on CSR data (pmf_svd_csr.h, pmf_host_svd_csr.h): v_csr with both CSR images resident and no dV, as on a CUR / CMD
  // context (cur_ip: the row pointers on the host).  Float64 throughout: the projected side [long side padded][svd_rp], rp = the
  // kept count rounded up to 64 (V is kept transposed for rows <= cols); PCA's W [mp][svd_wp] and H^T [np][svd_wp] -- dW and dH
  // are not used while CSR data is resident
  int svd_triples = 0;          // pmf_set_option("svd_num_triples"): leading triples a decomposition of CSR data keeps, 0 = all above the cut
  double *dSvdPd = nullptr, *dSvdWd = nullptr, *dSvdHTd = nullptr;
  int svd_rp = 0, svd_wp = 0;
  bool svd_fact = false;        // pmf_svd_decompose ran last: the factors of pmf_frobenius are W = U, H = S V of dSvdE / dSvdPd.  <- V, W, H
  // CUR / CMD (pmf_cur.h): the unscaled gathers Cg [mp][round_up(nc, 64)] and Rg [round_up(nr, 64)][np] of the last pmf_cur_compute;
  // on the host sqrt(ccnt), sqrt(rcnt) and the middle factor U [nc][nr]
  float *dCurCg = nullptr, *dCurRg = nullptr;
  int cur_nr = 0, cur_nc = 0;
  std::vector<double> cur_dc, cur_dr, cur_U;
  bool cur_valid = false;       // they belong to the current V.  <- V
  int opt_profile_cur = 0;      // pmf_set_option("profile_cur"): pmf_profile_enable times 0 the cross product, 1 k_lev_f64, 2 k_cur_sqnorms
  int opt_profile_vq = 0;       // pmf_set_option("profile_vq"): pmf_profile_enable times 0 the context's own kernel, 1 k_vq_pass, 2 k_vq_argmin_rows (pmf_vq.h)
  // pmf_set_v_gather_f32 (pmf_gather.h, pmf_host_gather.h), on the DESTINATION context: the index array as the kernel reads it, the
  // events that order the source's stream against the kernel (0: the source's work before it, 1: the kernel before the source's next)
  int32_t* dGaIdx = nullptr;
  int64_t ga_idx_cap = 0;
  hipEvent_t ev_ga[2] = {nullptr, nullptr};
  int opt_profile_gather = 0;   // pmf_set_option("profile_gather"): pmf_profile_enable times k_gather_cols, on any context
  // CUR / CMD on CSR data (pmf_cur_csr.h, pmf_host_cur_csr.h): v_csr with both CSR images resident (dIndptr ..., dTIndptr ...) and no
  // dV; on the host the row pointers (the chunk count of k_cur_csr_mid follows the longest selected row), ||data||^2 as the sum
  // of the row norms in row order, and the error of the last pmf_cur_compute by the trace identity (pmf_cur_ferr)
  std::vector<int64_t> cur_ip;
  double cur_vnorm2 = 0.0, cur_ferr = 0.0;
  bool cur_vnorm2_valid = false;   // <- V
  bool cur_ferr_valid = false;     // <- V (with cur_valid)
  // GREEDY / GREEDYCUR (pmf_greedy.h): the float64 Gram matrix on the short side of V and the rows of its eigenvectors ([qp][qp]
  // each), on the host the eigenvalues and the indices of those above svd.py's 1e-8 cut in descending order; pinv(W)^T [mp][KP]
  // float32, the operand of H = pinv(W) data.  The selection itself is read through dSvSel / sv_have_select (SIVM's).
  double *dGrG = nullptr, *dGrQT = nullptr;
  float* dGrMT = nullptr;
  std::vector<double> gr_ev;
  std::vector<int> gr_ord;
  bool gr_eig_valid = false;    // they belong to the current V.  <- V
  // GREEDY on CSR data (pmf_greedy_csr.h, pmf_host_greedy_csr.h): v_csr with both CSR images resident and no dV, as on a CUR / CMD
  // context; the H step's result as H^T [np][64] float64 -- dH is not written while CSR data is resident
  double* dGrHTd = nullptr;
  bool gr_ht_valid = false;     // dGrHTd holds the context's H (off: dH does).  <- H
  double lamb_w = 0.0, lamb_h = 0.0;   // BNMF penalty weights (bnmf.py:84-85,118-119)
  // streamed V (pmf_stream_*): row tiles pass through two device buffers, V is never resident
  float* dTile[2] = {nullptr, nullptr};
  int64_t tile_cap = 0;                      // rows per tile buffer (multiple of 64)
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
  double* dPSacc = nullptr;                  // float64 (P | S) accumulated over the tiles of a pass
  double* dStAcc = nullptr;                  // [0] sum v^2, [1] sum (v - (W H))^2 over the tiles
  bool st_active = false, st_vnorm_pending = false;
  uint32_t st_flags = 0;
  int64_t st_rows_seen = 0;
  int st_tiles = 0;
  // one-shot all-reduce over IPC-mapped receive areas (pmf_ipc.h): payloads <= PMF_IPC_MAX_BYTES
  IpcPeers ipc{};                            // ipc.nranks > 1: ready
  bool ipc_exported = false;
  unsigned long long ipc_wait_ticks = PMF_IPC_WAIT_TICKS;
  int ipc_nranks_ready = 0;                  // ranks mapped by pmf_ipc_import (ipc.nranks = 0 while the path is switched off)
  int ipc_export_nranks = 0;                 // the rank count pmf_ipc_export sized the receive area for
  float *dIpcTestA = nullptr, *dIpcTestB = nullptr;   // pmf_ipc_selftest's payloads, allocated by pmf_ipc_export (no allocation -- nothing
                                                      // that can fail locally -- between the self-test's collectives)
  unsigned ipc_seq = 0;
  std::atomic<int> abort_flag{0};            // pmf_abort: another host thread asks the running pmf_factorize loop to return early
  // the folded exchange (round 5): inside pmf_factorize's one-pass loop the push rides on k_reduce_slabs_tiles and the wait +
  // rank-ordered sum on k_nmf_h_gram's prologue -- no launch for the exchange (pmf_set_option("fold_exchange", 0): the
  // k_ipc_allreduce launch of round 4 instead)
  int opt_fold = 1;
  bool fold_loop = false;                    // set by nmf_fused_iteration around its two launches
  unsigned fold_seq = 0;                     // != 0: k_reduce_slabs_tiles has pushed exchange fold_seq, the next k_nmf_h_gram consumes it
  int fold_flags = 0;                        // tiles (= flags) of that push
  unsigned long long* dIpcWait = nullptr;    // [2]: ticks of the 100 MHz counter the consumer spent waiting, exchanges counted
  int64_t fold_calls = 0;
  int* dIpcErr = nullptr;
  int64_t coll_seen = 0;
  int64_t ipc_calls = 0, rccl_calls = 0, host_calls = 0;   // which transport the cross-rank sums took (pmf_collective_name)
  pmf_host_allreduce_fn host_ar = nullptr;   // host transport for the cross-rank sums (pmf_set_host_allreduce)
  void* host_ar_user = nullptr;
  std::vector<unsigned char> ar_buf;
  bool profile = false;
  std::vector<hipEvent_t> coll_ev;           // event pairs around the per-iteration collective (allreduce_ps)
  size_t coll_used = 0;
  bool host_ar_only() const { return host_ar != nullptr && ipc.nranks <= 1 && comm == nullptr; }   // (blocking host round trips: nothing to time on the stream)
  double last_loop_ms = 0.0;
  KernelStat stat;
  std::string err;
  std::string path;
};

namespace {

int fail(pmf_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg; else g_create_error = msg;
  return code;
}

#define HIPCHK(c, expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail((c), e_ == hipErrorOutOfMemory ? PMF_ENOMEM : PMF_EHIP,                 \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                     \
  } while (0)

#define NCCLCHK(c, expr)                                                                  \
  do {                                                                                    \
    ncclResult_t r_ = (expr);                                                             \
    if (r_ != ncclSuccess)                                                                \
      return fail((c), PMF_ENCCL, std::string(#expr) + ": " + ncclGetErrorString(r_));    \
  } while (0)

#define PMFCHK(expr)                 \
  do {                               \
    int rc_ = (expr);                \
    if (rc_ != PMF_OK) return rc_;   \
  } while (0)

int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// defined further down the include order
bool multi_rank(const pmf_ctx* c);
int csr_ps(pmf_ctx* c);
int csr_w(pmf_ctx* c, hipStream_t stream, const float* Mbuf, int reserve);
int materialize_w(pmf_ctx* c);
int nmf_fused_pass(pmf_ctx* c);
int snmf_fused_pass(pmf_ctx* c);
int snmf_inverse(pmf_ctx* c);
int ensure_ps(pmf_ctx* c);
int nmf_csr_sync_h(pmf_ctx* c);
void choose_stat_site(pmf_ctx* c, bool gram);

// ---- device memory: every buffer of a context is allocated, grown and released here ----------
// (the IPC receive area alone lives outside c->owned: it is allocated for export and peers hold handles to it)
// `bytes` of device memory as hipMalloc leaves them: nothing on the stream
int dalloc_raw(pmf_ctx* c, void** p, size_t bytes) {
  void* q = nullptr;
  HIPCHK(c, hipMalloc(&q, bytes));
  if (q) c->owned.push_back(q);
  *p = q;
  return PMF_OK;
}
template <typename T>
int dalloc_raw(pmf_ctx* c, T** p, size_t count) { return dalloc_raw(c, reinterpret_cast<void**>(p), count * sizeof(T)); }

// `count` elements, zero filled in stream order
template <typename T>
int dalloc(pmf_ctx* c, T** p, size_t count) {
  PMFCHK(dalloc_raw(c, p, std::max<size_t>(count, 1)));
  HIPCHK(c, hipMemsetAsync(*p, 0, std::max<size_t>(count, 1) * sizeof(T), c->stream));
  return PMF_OK;
}

// (hipFree waits for the device; a site whose buffer may still be read by work in flight synchronizes its stream first)
template <typename T>
int dfree(pmf_ctx* c, T** p) {
  if (!*p) return PMF_OK;
  void* q = (void*)*p;
  *p = nullptr;
  c->owned.erase(std::remove(c->owned.begin(), c->owned.end(), q), c->owned.end());
  HIPCHK(c, hipFree(q));
  return PMF_OK;
}

// a buffer that has become too small: released, then `count` zero filled elements
template <typename T>
int dgrow(pmf_ctx* c, T** p, size_t count) {
  PMFCHK(dfree(c, p));
  return dalloc(c, p, count);
}
// ... with a capacity field of its own: `*cap` x `per` elements held, `count` x `per` wanted; sync: work in flight may read the old one
template <typename T>
int dgrow(pmf_ctx* c, T** p, int64_t* cap, int64_t count, size_t per = 1, bool sync = false) {
  if (*cap >= count) return PMF_OK;
  if (sync && *p) HIPCHK(c, hipStreamSynchronize(c->stream));
  *cap = 0;
  PMFCHK(dgrow(c, p, (size_t)count * per));
  *cap = count;
  return PMF_OK;
}

// CSR kernels serve the data paths (SNMF and NMF, num_bases <= 128); wider SNMF contexts keep a dense image of the CSR rows
static inline bool use_csr(const pmf_ctx* c) { return c->v_csr && !c->csr_dense; }
// NMF on CSR data: both half steps are k_nmf_sp_step (pmf_host_nmf_csr.h)
static inline bool nmf_csr(const pmf_ctx* c) { return c->algo == PMF_ALGO_NMF && use_csr(c); }

// PCA / SVD contexts: the float32 factor W and the two scratch arrays of its shape, [rows padded][KP] each -- as large as the dense
// image when the context is as wide as the short side.  Allocated by the entry points that bring dense data or a float32-path W
// (pmf_set_v_dense_*, pmf_fill_v_uniform, pmf_set_w_*, pmf_fill_w_uniform), never while the context only ever holds CSR data.
int ensure_wbufs(pmf_ctx* c) {
  if (c->algo != PMF_ALGO_PCA) return PMF_OK;
  if (!c->dW) PMFCHK(dalloc(c, &c->dW, (size_t)c->mp * c->KP));
  if (!c->dW1) PMFCHK(dalloc(c, &c->dW1, (size_t)std::max<int64_t>(c->mp, c->np) * c->KP));
  if (c->nb > 1 && !c->dW2) PMFCHK(dalloc(c, &c->dW2, (size_t)c->mp * c->KP));
  return PMF_OK;
}

int ensure_dv(pmf_ctx* c) {
  if (c->dV) return PMF_OK;
  return dalloc(c, &c->dV, (size_t)c->mp * c->np);
}

// ---- profiling of the dominant kernel -------------------------------------------------
// Does this launch of the profiled site carry events (every N-th does)?  If so, s.ev[s.used] and s.ev[s.used + 1] exist on return.
bool stat_next_pair(KernelStat& s) {
  if (s.seen++ % s.every != 0) return false;
  while (s.used + 2 > s.ev.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return false;
    s.ev.push_back(e);
  }
  return true;
}
void stat_begin(pmf_ctx* c, int site) {
  if (!c->profile || c->stat.site != site) return;
  KernelStat& s = c->stat;
  s.open = false;
  if (!stat_next_pair(s)) return;
  (void)hipEventRecord(s.ev[s.used], c->stream);   // profiling aid: a failed record only loses a sample
  s.open = true;
}
// The next pair of events of site `site`, to be attached to a dispatch (hipExtLaunchKernelGGL); nullptr when not profiling.
void stat_pair(pmf_ctx* c, int site, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!c->profile || c->stat.site != site) return;
  KernelStat& s = c->stat;
  if (!stat_next_pair(s)) return;
  *e0 = s.ev[s.used]; *e1 = s.ev[s.used + 1];
  s.used += 2;
}
void stat_end(pmf_ctx* c, int site) {
  if (!c->profile || c->stat.site != site) return;
  KernelStat& s = c->stat;
  if (!s.open || s.used + 2 > s.ev.size()) return;
  s.open = false;
  (void)hipEventRecord(s.ev[s.used + 1], c->stream);
  s.used += 2;
}

int need(pmf_ctx* c, bool v, bool w, bool h) {
  if (!c) return PMF_EINVAL;
  c->hd_synced = false;        // (a new API call: whoever wrote the float32 H since the last one is noticed by k_hd_sync)
  c->psd_fresh = false;
  if (v && !c->have_v) return fail(c, PMF_EINVAL, "V has not been set (pmf_set_v_*)");
  if (w && !c->have_w) return fail(c, PMF_EINVAL, "W has not been set (pmf_set_w_f32)");
  if (h && !c->have_h) return fail(c, PMF_EINVAL, "H has not been set (pmf_set_h_f32)");
  HIPCHK(c, hipSetDevice(c->device));
  return PMF_OK;
}

// ---- an operand came from outside: the "<-" table at the flags' declarations (pmf_ctx) written as code.  Every entry point that
// replaces V, W, H or CNMF's G calls one of these instead of writing flags; the transitions inside the algorithms stay where they happen.
void v_replaced(pmf_ctx* c) {
  c->vnorm_valid = c->vnorm_local_valid = c->ps_valid = c->num_valid = c->trace_ready = c->c_valid = false;
  c->cl_sums_valid = c->cl_err_valid = c->cl_mu_valid = false;
  c->svd_valid = false;
  c->cur_valid = c->cur_ferr_valid = c->cur_vnorm2_valid = false;
  c->gr_eig_valid = false;
}
void w_replaced(pmf_ctx* c, bool by_caller) {   // by_caller: uploaded or filled through the ABI (not the NNDSVD init, not a restored snapshot)
  c->have_w = true; c->ps_valid = c->num_valid = c->trace_ready = c->w_implicit = false;
  c->sw_valid = false;
  c->cl_err_valid = false;
  if (by_caller) c->gs_started = false;           // (SIVM_GSAT: the walk starts again from the caller's vertices)
  if (by_caller) c->cn_user_w = c->algo == PMF_ALGO_CNMF;   // (CNMF: the error is taken against this W until a G step rebinds it)
}
// hd_synced, hd_force: what the float64 H (SNMF, CNMF) is to the new float32 H -- written with it (true, false), the caller's float64
// values beside their rounding (false, false), or not written at all (false, true: all of it is widened at its next use)
void h_replaced(pmf_ctx* c, bool hd_synced, bool hd_force) {
  c->have_h = true; c->g_valid = c->num_valid = c->trace_ready = false; c->g_parts = 0; c->hd_synced = hd_synced; c->hd_force = hd_force;
  c->cl_err_valid = false;
  c->ht_valid = c->ht_newer = false;
  c->gr_ht_valid = false;
  if (c->algo == PMF_ALGO_CMEANS) c->cl_sums_valid = false;   // (Kmeans' sums follow the assignment, not H: kmeans.py:82-87)
}
void g_replaced(pmf_ctx* c) {        // CNMF
  c->have_g = true; c->cn_ab_valid = c->cn_l_valid = false;
  if (!c->cn_user_w) { c->have_w = true; c->w_implicit = true; }   // cnmf.py:102-103,175: W = data G unless the caller set one
}
// the factors stay, sums over the data are formed anew: RNMF's D replaced, or (transport) the cross-rank sums take another way
void sums_dropped(pmf_ctx* c, bool transport) {
  c->ps_valid = c->trace_ready = false;
  if (transport) c->vnorm_valid = c->c_valid = false;
}

}  // namespace
