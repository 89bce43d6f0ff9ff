// pmf_host_profile.h -- which launch site pmf_profile_enable times: choose_stat_site (KernelStat and the event brackets: pmf_host_ctx.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// Which launch site pmf_profile_enable times, with the ALGORITHMIC flops / bytes of ONE launch on THIS
// rank's rows and the flops the kernel really executes (symmetry of W^T W,
// reassociations) next to them.
void choose_stat_site(pmf_ctx* c, bool gram) {
  const double m = (double)c->m, n = (double)c->n, k = (double)c->k, nnz = (double)c->nnz;
  KernelStat& st = c->stat;
  const int old_site = st.site;
  st.site = SITE_NONE; st.name = "none"; st.flops = st.bytes = st.exec_flops = 0.0;
  char buf[96];
  if (c->opt_profile_gather) {                                    // any context: gather_stat writes the name and the figures of the launch at hand
    st.site = SITE_GATHER;
    st.name = "k_gather_cols<idx>";
  } else if (c->opt_profile_vq) {                                 // any context: vq_stat writes the name and the figures of the launch at hand
    st.site = c->opt_profile_vq == 1 ? SITE_VQ : SITE_VQ_ARGMIN;
    st.name = c->opt_profile_vq == 1 ? "k_vq_pass<l2>" : "k_vq_argmin_rows";
  } else if (c->opt_profile_sivm_rows && (c->algo == PMF_ALGO_SIVM || c->algo == PMF_ALGO_CUR)) {
    st.site = SITE_SIVM_ROWS;                                     // one round of the long-sample pass; pmf_sivm_select restates the
    st.name = "k_sivm_rowdist<l2>+k_sivm_rowstep";                // figures for the matrix, the side and the measure of the call
    st.flops = st.exec_flops = 3.0 * m * n;
    st.bytes = 4.0 * m * (double)c->np;
  } else if (c->algo == PMF_ALGO_KMEANS || c->algo == PMF_ALGO_CMEANS) {
    st.site = SITE_CLUSTER;
    snprintf(buf, sizeof(buf), "k_cluster_pass<%d,%s>", c->NT, c->algo == PMF_ALGO_KMEANS ? "kmeans" : "cmeans");
    st.name = buf;
    st.flops = st.exec_flops = 4.0 * m * n * k;                  // W^T V and V H^T
    st.bytes = 4.0 * (m * n + k * n + 2.0 * m * k);              // V once, H written, W read, the sums written
    if (c->v_csr) {                                               // the two passes over stored entries: cluster_csr_update_h / _w write the
      snprintf(buf, sizeof(buf), "k_cluster_csr_assign<%d,%s>", c->k <= 64 ? 1 : 2, c->algo == PMF_ALGO_KMEANS ? "kmeans" : "cmeans");
      st.name = buf;                                              // name and the figures of the launch at hand
      st.flops = st.exec_flops = 2.0 * nnz * k;
      st.bytes = 8.0 * nnz + 16.0 * n + 8.0 * (c->k <= 64 ? 64.0 : 128.0) * n;
    }
  } else if (c->algo == PMF_ALGO_SIVM && c->sv_sgreedy) {
    st.site = SITE_SGREEDY;
    st.name = "k_sgreedy_pass";
    // round t = 1 .. k - 1: the differences as k_laesa_pass<l2>; the form's (t + 1)^2 products for each column
    // bytes: V once, the new table row written, rows 0 .. t - 2 read back -- the mean over the rounds
    double fl = 0.0, by = 0.0;
    for (int t = 1; t < c->k; ++t) {
      fl += 3.0 * m * n + 2.0 * (double)(t + 1) * (double)(t + 1) * n;
      by += 4.0 * m * (double)c->np + 4.0 * (double)c->np + 4.0 * (double)(t - 1) * (double)c->np;
    }
    st.flops = st.exec_flops = c->k > 1 ? fl / (double)(c->k - 1) : 0.0;
    st.bytes = c->k > 1 ? by / (double)(c->k - 1) : 0.0;
  } else if (c->algo == PMF_ALGO_SIVM && c->sv_rule == 1) {
    st.site = SITE_LAESA;
    snprintf(buf, sizeof(buf), "k_laesa_pass<%s>", c->sv_metric == 0 ? "l2" : c->sv_metric == 1 ? "l1" : "cosine");
    st.name = buf;
    st.flops = st.exec_flops = 3.0 * m * n;                       // difference, square, sum
    st.bytes = 4.0 * m * (double)c->np + 16.0 * (double)c->np;   // V once; one float64 state array read and written
  } else if (c->algo == PMF_ALGO_SIVM && c->sv_rule == 2) {
    st.site = SITE_GMAP;
    snprintf(buf, sizeof(buf), "k_gmap_pass<%s>", c->sv_gmap_method == 0 ? "pca" : c->sv_gmap_method == 1 ? "aa" : "nmf");
    st.name = buf;
    st.flops = st.exec_flops = 2.0 * m * n;                       // product, sum
    st.bytes = 4.0 * m * (double)c->np + 24.0 * (double)c->np;   // (rounds >= 1) V once; the norms read, iterval read and written
  } else if (c->algo == PMF_ALGO_SIVM) {
    st.site = SITE_SIVM;
    snprintf(buf, sizeof(buf), "k_sivm_pass<%s>", c->sv_metric == 0 ? "l2" : c->sv_metric == 1 ? "l1" : "cosine");
    st.name = buf;
    st.flops = st.exec_flops = 3.0 * m * n;                       // difference, square, sum
    st.bytes = 4.0 * m * (double)c->np + 48.0 * (double)c->np;   // V once; three float64 state arrays read and written
  } else if (c->algo == PMF_ALGO_AA) {
    st.site = SITE_AA;
    snprintf(buf, sizeof(buf), "k_aa_price<%d>", c->NT);
    st.name = buf;
    st.flops = st.exec_flops = 2.0 * m * n * k;                   // G = R^T V
    st.bytes = 4.0 * m * (double)c->np;                          // V once
  } else if (c->algo == PMF_ALGO_PCA) {
    st.site = SITE_SVD;
    const bool left = c->m > c->n;
    st.name = left ? "k_prod_f64<true,sym>" : "k_prod_f64<false,sym>";
    const double q = left ? n : m;
    st.flops = 2.0 * m * n * q;                                   // the whole Gram matrix ...
    st.exec_flops = m * n * (q + 64.0);                           // ... of which the upper block triangle is formed
    st.bytes = 4.0 * (double)c->mp * (double)c->np;              // V once
    if (c->v_csr) {                                               // the projection pass: svd_csr_proj writes the figures of the launch
      st.name = "k_csr_proj_f64";
      st.flops = st.exec_flops = 2.0 * nnz * 64.0;
      st.bytes = 12.0 * nnz + 8.0 * (double)(c->m > c->n ? c->mp : (int64_t)c->np) * 65.0;
    }
  } else if (c->algo == PMF_ALGO_CUR && c->opt_profile_cur == 1) {
    st.site = SITE_CUR_LEV;                                       // the long-side leverage pass: cur_leverage writes the instantiation's name
    st.name = "k_lev_f64";                                        // and the flops and bytes of the call (they depend on its k)
  } else if (c->algo == PMF_ALGO_CUR && c->opt_profile_cur == 2) {
    st.site = SITE_CUR_SQNORMS;
    st.name = "k_cur_sqnorms";
    st.flops = st.exec_flops = 3.0 * m * n;                       // one square, a row sum and a column sum per value
    st.bytes = 4.0 * (double)c->mp * (double)c->np + 8.0 * (double)c->mp * (double)c->np * (1.0 / 256.0 + 1.0 / 64.0);   // V once, the partials
  } else if (c->algo == PMF_ALGO_CUR) {
    st.site = SITE_CUR;                                           // (nr = nc = the context's k assumed: the call may pass fewer)
    const bool trans = c->m > c->n;
    st.name = trans ? "k_prod_f64<true,full>" : "k_prod_f64<false,full>";
    st.flops = st.exec_flops = 2.0 * m * n * k;                   // T = V Rg^T or T' = Cg^T V
    const double kp = (double)round_up(c->k, 64);                // V once and the gathered operand once: Rg [kp][np] or Cg [mp][kp]
    st.bytes = 4.0 * (double)c->mp * (double)c->np + 4.0 * kp * (trans ? (double)c->mp : (double)c->np);
  } else if (c->algo == PMF_ALGO_GREEDY) {
    st.site = SITE_GREEDY;                                        // (rows <= cols: the last round's pass, 2 k - 1 operand columns)
    snprintf(buf, sizeof(buf), "k_greedy_pass<%d>", std::max(1, (2 * c->k - 1 + 15) / 16));
    st.name = buf;
    st.flops = st.exec_flops = 2.0 * m * n * (2.0 * k - 1.0);     // [B' | Q]^T V
    st.bytes = 4.0 * m * (double)c->np + 9.0 * (double)c->np;    // V once; the norms and the flags of the chosen columns
    if (c->v_csr) {                                               // the pass over stored entries: greedy_csr_rounds writes the figures of the launch
      st.name = "k_greedy_csr_pass<2>";
      st.flops = st.exec_flops = 2.0 * nnz * (2.0 * k - 1.0);
      st.bytes = 12.0 * nnz + 8.0 * n + 4.0 * 128.0 * m;
    }
  } else if (c->algo == PMF_ALGO_SNMF && gram) {
    st.site = SITE_MATERIALIZE;                   // the only m-sized kernel of a Gram-space loop: W = V M, once
    if (use_csr(c)) {
      st.name = "k_csr_w_blocks(W = V M)";
      st.flops = st.exec_flops = 2.0 * nnz * k;
      st.bytes = 4.0 * m * k + 8.0 * nnz + 8.0 * (m + 1.0);      // W written once; CSR arrays read once
    } else {
      snprintf(buf, sizeof(buf), "k_rowgemm<%d,store>(W = V M^T)", c->NT);
      st.name = buf;
      st.flops = st.exec_flops = 2.0 * m * n * k;
      st.bytes = 4.0 * (m * n + m * k);
    }
  } else if (c->algo == PMF_ALGO_SNMF && use_csr(c)) {
    st.site = SITE_CSR_PASS;
    st.name = "k_snmf_csr_pass";                  // until the first launch: launch_csr_mfma / launch_csr_fused name their instantiation
    st.flops = 4.0 * nnz * k + 4.0 * m * k * k;                  // SURVEY: SpMM, (.) inv, W^T V, W^T W
    st.exec_flops = 4.0 * nnz * k + m * k * (k + 16.0);          // V M, W^T V, upper triangle of W^T W
    st.bytes = 4.0 * m * k + 8.0 * nnz + 8.0 * (m + 1.0);
  } else if (nmf_csr(c)) {
    st.site = SITE_CSR_PASS;                      // both half steps of an iteration, alternating; the figures are the W step's
    snprintf(buf, sizeof(buf), "k_nmf_sp_step<%d>", c->NT);
    st.name = buf;
    const double kp = (double)c->KP;
    st.flops = 2.0 * nnz * k + 4.0 * m * k * k;                  // the gather, X G, X^T X
    st.exec_flops = 2.0 * nnz * kp + 2.0 * m * kp * kp + m * kp * (kp + 16.0);
    st.bytes = 12.0 * nnz + 8.0 * m * kp + 4.0 * nnz * kp;       // CSR arrays once, X read and written, the gathered rows of Y
  } else if (c->fused_wgs > 0 && c->algo != PMF_ALGO_NMFALS) {
    st.site = SITE_FUSED;
    st.name = c->fused8 ? c->path.c_str()
                        : pmf_fused_kernel_name(c->NT, c->np, c->algo == PMF_ALGO_SNMF   ? FUSED_SNMF
                                                          : c->algo == PMF_ALGO_BNMF ? FUSED_BNMF
                                                          : c->algo == PMF_ALGO_RNMF ? FUSED_RNMF
                                                                                     : FUSED_NMF);
    // one pass over V does the four m-sized contractions of an iteration: F = 4 m n k + 4 m k^2
    st.flops = 4.0 * m * n * k + 4.0 * m * k * k;
    if (c->algo == PMF_ALGO_SNMF) {               // executes V M^T, W^T V and the upper triangle of W^T W
      st.exec_flops = 4.0 * m * n * k + m * k * (k + 16.0);
      st.bytes = 4.0 * (m * n + m * k);           // V read once, W written once
    } else if (c->fused8) {                       // V H^T, W G, W^T V and ALL of W^T W (base split: no symmetry to use)
      st.exec_flops = 4.0 * m * n * k + 4.0 * m * k * k;
      st.bytes = 4.0 * (m * n + 2.0 * m * k);
    } else {                                      // V H^T, W G, W^T V and the upper triangle of W^T W
      st.exec_flops = 4.0 * m * n * k + 2.0 * m * k * k + m * k * (k + 16.0);
      st.bytes = 4.0 * (m * n + 2.0 * m * k);     // V read once, W read and written once
    }
  } else if (c->algo == PMF_ALGO_NMFALS) {
    st.site = SITE_NNQP_W;
    if (c->opt_nnqp_quad && c->k <= 64 && (c->m >= 16384 || c->opt_nnqp_quad == 2)) snprintf(buf, sizeof(buf), "k_nnqp_quad(update_w)");
    else if (c->k <= 64) snprintf(buf, sizeof(buf), "k_nnqp<%d>(update_w)", c->k <= 16 ? 16 : c->k <= 32 ? 32 : 64);
    else if (nnqp_use_wave(c)) snprintf(buf, sizeof(buf), "k_nnqp_wave(update_w)");
    else snprintf(buf, sizeof(buf), "k_nnqp_big<%d>(update_w)", pmf_nnqp_big_vpl(c->k));
    st.name = buf;
    st.bytes = 4.0 * (3.0 * m * k);               // right-hand sides read, warm start read, solution written
  } else if ((c->algo == PMF_ALGO_NMF) && c->nb == 1) {
    st.site = SITE_ROWGEMM_W;
    snprintf(buf, sizeof(buf), "k_rowgemm<%d,nmf_w>", c->NT);
    st.name = buf;
    st.flops = st.exec_flops = 2.0 * m * n * k + 2.0 * m * k * k;
    st.bytes = 4.0 * (m * n + 2.0 * m * k);
  }
  if (st.site != old_site) st.used = 0;
}

}  // namespace
