// pmf_host_cluster_csr.h -- Kmeans / Cmeans on CSR data: the checked upload with its transposed copy, the H step over the samples,
// the W step over the chunks of the data rows, the error (kernels: pmf_cluster_csr.h, pmf_cluster.h, pmf_cur_csr.h, pmf_svd_csr.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
//
// State (pmf_ctx): v_csr on a Kmeans / Cmeans context = both CSR images resident (dIndptr ... of V, dTIndptr ... of V^T) and no dense
// V: dV and the dense path's slabs are released by the upload.  W is dW (float32).  H lives as H^T [np][cc_ld] float64 in dCcHT:
// pmf_get_h_* / pmf_set_h_* transpose on the way, dH is not read or written.  The assignment (dClAsg) and the flags cl_have_asg,
// cl_sums_valid (here: dCcTot holds the denominators of the assignment / H at hand), cl_err_valid are the dense path's, with its
// pairing: an H step leaves the denominators that the next W step divides by; a W step that no pass preceded forms them first.
#pragma once

namespace {

// the entry points that have no CSR form on a Kmeans / Cmeans context
int cluster_csr_refuse(pmf_ctx* c, const char* who) {
  if (!c || !cluster_csr(c)) return PMF_OK;
  return fail(c, PMF_EINVAL, std::string(who) + ": not while CSR data is resident on a Kmeans / Cmeans context (pmf_update_w, pmf_update_h, "
                                                "pmf_factorize, pmf_frobenius, pmf_cluster_get_assigned, pmf_cluster_set_assigned and the "
                                                "factor transfers work on it; dense data brings the rest back)");
}

int cluster_csr_nh(const pmf_ctx* c) { return c->k <= 64 ? 1 : 2; }

const char* cluster_csr_kernel_name(const pmf_ctx* c, const char* stem, char* buf, size_t len) {
  snprintf(buf, len, "%s<%d,%s>", stem, cluster_csr_nh(c), c->algo == PMF_ALGO_KMEANS ? "kmeans" : "cmeans");
  return buf;
}

int cluster_csr_ht(pmf_ctx* c, bool to_h) {
  const int64_t elems = (int64_t)c->np * c->cc_ld;
  hipLaunchKernelGGL(k_cluster_csr_ht, dim3(elem_grid(elems)), dim3(256), 0, c->stream, c->dH, c->np, c->k, c->cc_ld, elems, c->dCcHT, to_h ? 1 : 0);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// dense data came back to the context: the CSR arrays and their side arrays go, H is rounded into dH
int cluster_csr_left(pmf_ctx* c) {
  if (!is_cluster(c) || !c->dIndptr) return PMF_OK;
  if (c->have_h && c->dCcHT) PMFCHK(cluster_csr_ht(c, true));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dIndptr));
  PMFCHK(dfree(c, &c->dIndices));
  PMFCHK(dfree(c, &c->dVals));
  PMFCHK(dfree(c, &c->dTIndptr));
  PMFCHK(dfree(c, &c->dTIndices));
  PMFCHK(dfree(c, &c->dTVals));
  PMFCHK(dfree(c, &c->dCcHT));
  PMFCHK(dfree(c, &c->dCcSq));
  PMFCHK(dfree(c, &c->dCcPart));
  PMFCHK(dfree(c, &c->dCcDen));
  PMFCHK(dfree(c, &c->dCcErr));
  PMFCHK(dfree(c, &c->dCcTot));
  PMFCHK(dfree(c, &c->dCcWn));
  PMFCHK(dfree(c, &c->dCcChunkOff));
  PMFCHK(dfree(c, &c->dCcChunkRow));
  c->nnz = 0; c->v_csr = false;
  c->cc_chunks = c->cc_wgs = c->cc_lpw = 0;
  c->cl_sums_valid = c->cl_err_valid = false;
  c->path = "cluster_panels";
  choose_stat_site(c, false);
  return PMF_OK;
}

// pmf_set_v_csr_f32 on a Kmeans / Cmeans context: refused arrays never reach the device and leave the resident data as it was
int cluster_csr_set_v(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz) {
  if (c->nranks > 1 || multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_set_v_csr_f32: Kmeans / Cmeans on CSR data: one rank only in this build");
  const char* why = csr_check(c->m, c->n, indptr, indices, nnz);
  if (!why) why = csr_check_ascending(c->m, indptr, indices);
  if (why) return fail(c, PMF_EINVAL, std::string("pmf_set_v_csr_f32: ") + why);
  // the chunks of the data rows, numbered row by row: the launch shape of the W step follows from indptr alone
  std::vector<int> off((size_t)c->mp + 1, 0);
  int64_t total = 0;
  for (int64_t r = 0; r < c->m; ++r) {
    off[(size_t)r] = (int)total;
    total += (indptr[r + 1] - indptr[r] + PMF_CCSR_CHUNK - 1) / PMF_CCSR_CHUNK;
    if (total > 0x7ffffff0) return fail(c, PMF_EINVAL, "pmf_set_v_csr_f32: Kmeans / Cmeans on CSR data: too many stored entries for this build");
  }
  for (int64_t r = c->m; r <= c->mp; ++r) off[(size_t)r] = (int)total;
  std::vector<int> rows((size_t)total);
  for (int64_t r = 0; r < c->m; ++r)
    for (int g = off[(size_t)r]; g < off[(size_t)r + 1]; ++g) rows[(size_t)g] = (int)r;
  CsrPair p;
  csr_transpose_host(c, indptr, indices, vals, nnz, p);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int ld = 64 * cluster_csr_nh(c);
  c->cc_ld = ld;
  if (!c->dCcHT) {
    PMFCHK(dalloc(c, &c->dCcHT, (size_t)c->np * ld));
    if (c->have_h) PMFCHK(cluster_csr_ht(c, false));    // (the H of the dense path at hand, widened)
  }
  c->cc_lpw = (int)round_up(std::max<int64_t>(PMF_CCSR_MIN_LINES, (c->n + PMF_CL_MAX_WGS - 1) / PMF_CL_MAX_WGS), 4);
  c->cc_wgs = (int)((c->n + c->cc_lpw - 1) / c->cc_lpw);
  if (!c->dCcSq) PMFCHK(dalloc(c, &c->dCcSq, (size_t)(c->mp + c->np)));
  if (!c->dCcDen) PMFCHK(dalloc(c, &c->dCcDen, (size_t)c->cc_wgs * ld));
  if (!c->dCcErr) PMFCHK(dalloc(c, &c->dCcErr, (size_t)c->cc_wgs * 2));
  if (!c->dCcTot) PMFCHK(dalloc(c, &c->dCcTot, (size_t)ld + 2));
  if (!c->dCcWn) PMFCHK(dalloc(c, &c->dCcWn, (size_t)ld));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dV));                            // a CSR upload replaces dense data ...
  PMFCHK(dfree(c, &c->dClNum));                        // ... and the slabs of the pass over it (cluster_alloc brings them back)
  PMFCHK(csr_upload_pair(c, p, indices, vals, nnz));
  c->cc_chunks = 0;
  PMFCHK(dgrow(c, &c->dCcChunkOff, off.size()));
  PMFCHK(dgrow(c, &c->dCcChunkRow, rows.size()));
  PMFCHK(dgrow(c, &c->dCcPart, (size_t)total * ld));
  HIPCHK(c, hipMemcpyAsync(c->dCcChunkOff, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (total) HIPCHK(c, hipMemcpyAsync(c->dCcChunkRow, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (c->np > c->n)                                    // pad samples: -1, as the dense pass leaves them
    HIPCHK(c, hipMemsetAsync(c->dClAsg + c->n, 0xFF, (size_t)(c->np - c->n) * sizeof(int), c->stream));
  c->cc_chunks = (int)total;
  c->nnz = nnz; c->have_v = true; c->v_csr = true; c->csr_dense = false;
  v_replaced(c);
  // |v|^2 of every row and sample and ||V||^2 (the row norms added in row order on the host), once per upload
  constexpr int per_wg = 256 / PMF_CURSP_TEAM;
  const int64_t lines = c->mp + c->np;
  hipLaunchKernelGGL(k_cur_csr_sqnorms, dim3((unsigned)((lines + per_wg - 1) / per_wg)), dim3(256), 0, c->stream, (const int64_t*)c->dIndptr,
                     (const float*)c->dVals, c->mp, (const int64_t*)c->dTIndptr, (const float*)c->dTVals, (int64_t)c->np, c->dCcSq);
  HIPCHK(c, hipGetLastError());
  std::vector<double> sq((size_t)c->m);
  HIPCHK(c, hipMemcpyAsync(sq.data(), c->dCcSq, sq.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));          // (the host arrays may leave scope)
  double s = 0.0;
  for (double v : sq) s += v;
  c->cur_vnorm2 = s;
  c->cur_vnorm2_valid = true;
  c->path = "cluster_csr";
  choose_stat_site(c, false);
  return PMF_OK;
}

template <int NH>
int cluster_csr_assign_t(pmf_ctx* c, const ClusterCsrArgs& a) {
  if (c->algo == PMF_ALGO_KMEANS)
    hipLaunchKernelGGL((k_cluster_csr_assign<NH, PMF_CL_KMEANS>), dim3((unsigned)c->cc_wgs), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL((k_cluster_csr_assign<NH, PMF_CL_CMEANS>), dim3((unsigned)c->cc_wgs), dim3(256), 0, c->stream, a);
  return PMF_OK;
}

int cluster_csr_totals(pmf_ctx* c) {
  hipLaunchKernelGGL(k_cluster_totals, dim3(1), dim3(256), 0, c->stream, (const double*)c->dCcDen, (const double*)c->dCcErr, c->cc_wgs, c->cc_ld, c->dCcTot);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// the H step: assignment / memberships from the current W, with the denominators of the next W step
int cluster_csr_update_h(pmf_ctx* c) {
  const int ld = c->cc_ld;
  hipLaunchKernelGGL(k_cluster_csr_wnorm, dim3((unsigned)c->KP), dim3(256), 0, c->stream, (const float*)c->dW, c->mp, c->KP, c->dCcWn);
  HIPCHK(c, hipGetLastError());
  ClusterCsrArgs a{};
  a.indptr = c->dTIndptr; a.indices = c->dTIndices; a.vals = c->dTVals; a.W = c->dW; a.vn2 = c->dCcSq + c->mp; a.wn = c->dCcWn;
  a.HT = c->dCcHT; a.asg = c->dClAsg; a.pden = c->dCcDen; a.perr = c->dCcErr;
  a.lines = (int)c->n; a.lines_per_wg = c->cc_lpw; a.k = c->k; a.KP = c->KP;
  if (c->profile && c->stat.site == SITE_CLUSTER) {     // the record of the launch at hand
    char buf[96];
    c->stat.name = cluster_csr_kernel_name(c, "k_cluster_csr_assign", buf, sizeof(buf));
    c->stat.flops = c->stat.exec_flops = 2.0 * (double)c->nnz * (double)c->k;
    // the entries, the pointers, |v|^2, the rows of H^T written (Kmeans: and the assignment); the rows of W come from L2
    c->stat.bytes = 8.0 * (double)c->nnz + 16.0 * (double)c->n + 8.0 * ld * (double)c->n + (c->algo == PMF_ALGO_KMEANS ? 4.0 * (double)c->n : 0.0);
  }
  stat_begin(c, SITE_CLUSTER);
  if (ld == 64) PMFCHK(cluster_csr_assign_t<1>(c, a));
  else PMFCHK(cluster_csr_assign_t<2>(c, a));
  stat_end(c, SITE_CLUSTER);
  HIPCHK(c, hipGetLastError());
  PMFCHK(cluster_csr_totals(c));
  h_replaced(c, false, true);
  if (c->algo == PMF_ALGO_KMEANS) c->cl_have_asg = true;
  c->cl_sums_valid = true;
  c->cl_err_valid = c->algo == PMF_ALGO_KMEANS;        // dCcTot[ld] = ||V - W H||^2 of the W, H at hand
  return PMF_OK;
}

// the denominators of the assignment (Kmeans) / H (Cmeans) at hand, in the order of the H step
int cluster_csr_den(pmf_ctx* c) {
  const dim3 grid((unsigned)c->cc_wgs);
  const int n = (int)c->n;
  if (c->cc_ld == 64) {
    if (c->algo == PMF_ALGO_KMEANS) hipLaunchKernelGGL((k_cluster_csr_den<1, PMF_CL_KMEANS>), grid, dim3(256), 0, c->stream, (const double*)c->dCcHT, (const int*)c->dClAsg, n, c->cc_lpw, c->dCcDen, c->dCcErr);
    else hipLaunchKernelGGL((k_cluster_csr_den<1, PMF_CL_CMEANS>), grid, dim3(256), 0, c->stream, (const double*)c->dCcHT, (const int*)c->dClAsg, n, c->cc_lpw, c->dCcDen, c->dCcErr);
  } else {
    if (c->algo == PMF_ALGO_KMEANS) hipLaunchKernelGGL((k_cluster_csr_den<2, PMF_CL_KMEANS>), grid, dim3(256), 0, c->stream, (const double*)c->dCcHT, (const int*)c->dClAsg, n, c->cc_lpw, c->dCcDen, c->dCcErr);
    else hipLaunchKernelGGL((k_cluster_csr_den<2, PMF_CL_CMEANS>), grid, dim3(256), 0, c->stream, (const double*)c->dCcHT, (const int*)c->dClAsg, n, c->cc_lpw, c->dCcDen, c->dCcErr);
  }
  HIPCHK(c, hipGetLastError());
  PMFCHK(cluster_csr_totals(c));
  c->cl_sums_valid = true;
  c->cl_err_valid = false;
  return PMF_OK;
}

template <int NH>
int cluster_csr_num_t(pmf_ctx* c) {
  const dim3 grid((unsigned)((c->cc_chunks + 3) / 4));
  if (c->algo == PMF_ALGO_KMEANS)
    hipLaunchKernelGGL((k_cluster_csr_num<NH, PMF_CL_KMEANS>), grid, dim3(256), 0, c->stream, (const int64_t*)c->dIndptr, (const int32_t*)c->dIndices,
                       (const float*)c->dVals, (const int*)c->dCcChunkRow, (const int*)c->dCcChunkOff, c->cc_chunks, (const double*)c->dCcHT,
                       (const int*)c->dClAsg, c->dCcPart);
  else
    hipLaunchKernelGGL((k_cluster_csr_num<NH, PMF_CL_CMEANS>), grid, dim3(256), 0, c->stream, (const int64_t*)c->dIndptr, (const int32_t*)c->dIndices,
                       (const float*)c->dVals, (const int*)c->dCcChunkRow, (const int*)c->dCcChunkOff, c->cc_chunks, (const double*)c->dCcHT,
                       (const int*)c->dClAsg, c->dCcPart);
  return PMF_OK;
}

// the W step: Num over the chunks of the data rows, divided by the denominators at hand
int cluster_csr_update_w(pmf_ctx* c) {
  if (c->algo == PMF_ALGO_KMEANS && !c->cl_have_asg)
    return fail(c, PMF_EINVAL, "Kmeans: update_w needs an assignment (update_h has not run)");
  if (!c->cl_sums_valid) PMFCHK(cluster_csr_den(c));
  const int ld = c->cc_ld;
  if (c->cc_chunks > 0) {
    if (c->profile && c->stat.site == SITE_CLUSTER) {
      char buf[96];
      c->stat.name = cluster_csr_kernel_name(c, "k_cluster_csr_num", buf, sizeof(buf));
      c->stat.flops = c->stat.exec_flops = 2.0 * (double)c->nnz * (double)c->k;
      // the entries, the pointers and chunk tables, the partials written; Kmeans: one word of the assignment per entry, Cmeans: one
      // row of H^T per entry (rows of a sample that several data rows store come from L2)
      c->stat.bytes = 8.0 * (double)c->nnz + 8.0 * (double)c->m + 8.0 * (double)c->cc_chunks + 8.0 * ld * (double)c->cc_chunks +
                      (c->algo == PMF_ALGO_KMEANS ? 4.0 : 8.0 * ld) * (double)c->nnz;
    }
    stat_begin(c, SITE_CLUSTER);
    if (ld == 64) PMFCHK(cluster_csr_num_t<1>(c));
    else PMFCHK(cluster_csr_num_t<2>(c));
    stat_end(c, SITE_CLUSTER);
    HIPCHK(c, hipGetLastError());
  }
  const int64_t elems = c->m * c->KP;
  if (c->algo == PMF_ALGO_KMEANS)
    hipLaunchKernelGGL(k_cluster_csr_finish<PMF_CL_KMEANS>, dim3(elem_grid(elems)), dim3(256), 0, c->stream, (const double*)c->dCcPart,
                       (const int*)c->dCcChunkOff, ld, elems, c->KP, c->k, (const double*)c->dCcTot, c->dW);
  else
    hipLaunchKernelGGL(k_cluster_csr_finish<PMF_CL_CMEANS>, dim3(elem_grid(elems)), dim3(256), 0, c->stream, (const double*)c->dCcPart,
                       (const int*)c->dCcChunkOff, ld, elems, c->KP, c->k, (const double*)c->dCcTot, c->dW);
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  c->cl_err_valid = false;
  return PMF_OK;
}

// ||V - W H||: Kmeans right behind its own assignment has it as sum_j min_c d^2 (float64 throughout: no cancellation guard is
// needed); everything else takes the float64 trace identity (svd_csr_err) on a float64 copy of W and on H^T
int cluster_csr_error(pmf_ctx* c, double* out) {
  const int ld = c->cc_ld;
  if (c->cl_err_valid) {
    double t = 0.0;
    HIPCHK(c, hipMemcpyAsync(&t, c->dCcTot + ld, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = std::sqrt(t > 0.0 ? t : 0.0);
    return PMF_OK;
  }
  DevTemps tmp;
  double* Wd = nullptr;
  PMFCHK(talloc(c, tmp, &Wd, (size_t)c->mp * ld));
  const int64_t elems = c->mp * ld;
  hipLaunchKernelGGL(k_cluster_csr_widen, dim3(elem_grid(elems)), dim3(256), 0, c->stream, (const float*)c->dW, c->KP, c->k, ld, elems, Wd);
  HIPCHK(c, hipGetLastError());
  return svd_csr_err(c, Wd, c->dCcHT, ld, ld, out);     // (synchronises: the temporary is released on return)
}

// the factor transfers of H while CSR data is resident: the caller's [k][n] layout, H^T on the device
template <typename T>
int cluster_csr_set_h(pmf_ctx* c, const T* H) {
  const int ld = c->cc_ld, k = c->k;
  const int64_t n = c->n;
  std::vector<double> h((size_t)n * ld, 0.0);
  for (int i = 0; i < k; ++i)
    for (int64_t col = 0; col < n; ++col) h[(size_t)col * ld + i] = (double)H[(size_t)i * n + col];
  HIPCHK(c, hipMemcpyAsync(c->dCcHT, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  h_replaced(c, false, true);
  return PMF_OK;
}

template <typename T>
int cluster_csr_get_h(pmf_ctx* c, T* H) {
  const int ld = c->cc_ld, k = c->k;
  const int64_t n = c->n;
  std::vector<double> h((size_t)n * ld);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->dCcHT, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < k; ++i)
    for (int64_t col = 0; col < n; ++col) H[(size_t)i * n + col] = (T)h[(size_t)col * ld + i];
  return PMF_OK;
}

}  // namespace
