// pmf_host_cur_csr.h -- CUR / CMD on CSR data: the checked upload with its transposed copy, the sampling norms, the gather and the
// middle product over stored entries, the error by the trace identity (kernels: pmf_cur_csr.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
//
// State (pmf_ctx): v_csr on a CUR / CMD context = both CSR images resident (dIndptr ... of V, dTIndptr ... of V^T: the fields of an
// NMF context on CSR data) and no dense V: dV is released by the upload, so every dense-only entry point finds no data.  The
// gathers Cg, Rg, the Gram matrices, the pseudo-inverses and the host finish are the dense path's (pmf_host_cur.h).
#pragma once

namespace {

bool cur_csr(const pmf_ctx* c) { return c->algo == PMF_ALGO_CUR && c->v_csr; }

// the entry points that have no CSR form on a CUR / CMD context
int cur_csr_refuse(pmf_ctx* c, const char* who) {
  if (!c || !cur_csr(c)) return PMF_OK;
  return fail(c, PMF_EINVAL, std::string(who) + ": not while CSR data is resident on a CUR / CMD context (pmf_cur_sqnorms, pmf_cur_compute, "
                                                "pmf_cur_get and pmf_cur_ferr work on it; dense data brings the rest back)");
}

// beyond csr_check: (a + b)^2 is not a^2 + b^2, so the norms need one entry per (row, column) pair
const char* csr_check_ascending(int64_t m, const int64_t* indptr, const int32_t* indices) {
  for (int64_t r = 0; r < m; ++r)
    for (int64_t e = indptr[r] + 1; e < indptr[r + 1]; ++e)
      if (indices[e] <= indices[e - 1]) return "column indices must ascend within a row, without duplicates (CUR / CMD)";
  return nullptr;
}

// dense data came back to the context: the CSR arrays go
int cur_csr_left(pmf_ctx* c) {
  if (c->algo != PMF_ALGO_CUR || !c->dIndptr) return PMF_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dIndptr));
  PMFCHK(dfree(c, &c->dIndices));
  PMFCHK(dfree(c, &c->dVals));
  PMFCHK(dfree(c, &c->dTIndptr));
  PMFCHK(dfree(c, &c->dTIndices));
  PMFCHK(dfree(c, &c->dTVals));
  std::vector<int64_t>().swap(c->cur_ip);
  c->nnz = 0; c->v_csr = false;
  c->path = "cur_cross_f64";
  choose_stat_site(c, false);
  return PMF_OK;
}

// pmf_set_v_csr_f32 on a CUR / CMD context: refused arrays never reach the device and leave the resident data as it was
int cur_csr_set_v(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz) {
  if (c->nranks > 1 || multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_set_v_csr_f32: CUR / CMD on CSR data: one rank only in this build");
  const char* why = csr_check(c->m, c->n, indptr, indices, nnz);
  if (!why) why = csr_check_ascending(c->m, indptr, indices);
  if (why) return fail(c, PMF_EINVAL, std::string("pmf_set_v_csr_f32: ") + why);
  CsrPair p;
  csr_transpose_host(c, indptr, indices, vals, nnz, p);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dV));                            // a CSR upload replaces dense data
  PMFCHK(csr_upload_pair(c, p, indices, vals, nnz));
  c->cur_ip.assign(indptr, indptr + c->m + 1);
  c->nnz = nnz; c->have_v = true; c->v_csr = true; c->csr_dense = false;
  v_replaced(c);
  c->path = "cur_csr";
  choose_stat_site(c, false);
  return PMF_OK;
}

// sqnorms_f64 on the stored entries: the row sums [mp] and, behind them, the column sums [np], pad positions 0
int cur_csr_sqnorms_f64(pmf_ctx* c, DevTemps& tmp, bool timed, double** sq) {
  const int64_t lines = c->mp + c->np;
  PMFCHK(talloc(c, tmp, sq, (size_t)lines));
  if (timed && c->profile && c->stat.site == SITE_CUR_SQNORMS) {
    c->stat.name = "k_cur_csr_sqnorms";
    c->stat.flops = c->stat.exec_flops = 4.0 * (double)c->nnz;                // a square and a sum, for the row and for the column
    c->stat.bytes = 8.0 * (double)c->nnz + 16.0 * (double)lines;              // the values twice, the pointers, the sums
  }
  constexpr int per_wg = 256 / PMF_CURSP_TEAM;
  if (timed) stat_begin(c, SITE_CUR_SQNORMS);
  hipLaunchKernelGGL(k_cur_csr_sqnorms, dim3((unsigned)((lines + per_wg - 1) / per_wg)), dim3(256), 0, c->stream, (const int64_t*)c->dIndptr,
                     (const float*)c->dVals, c->mp, (const int64_t*)c->dTIndptr, (const float*)c->dTVals, (int64_t)c->np, *sq);
  if (timed) stat_end(c, SITE_CUR_SQNORMS);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// ||data||^2 = the sum of the row norms in row order (host, float64); kept until the data change
int cur_csr_vnorm2(pmf_ctx* c, const double* row_sq_host) {
  if (c->cur_vnorm2_valid) return PMF_OK;
  std::vector<double> own;
  if (!row_sq_host) {
    DevTemps tmp;
    double* sq = nullptr;
    PMFCHK(cur_csr_sqnorms_f64(c, tmp, false, &sq));
    own.resize((size_t)c->m);
    HIPCHK(c, hipMemcpyAsync(own.data(), sq, own.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the temporary is released on return
    row_sq_host = own.data();
  }
  double s = 0.0;
  for (int64_t r = 0; r < c->m; ++r) s += row_sq_host[r];
  c->cur_vnorm2 = s;
  c->cur_vnorm2_valid = true;
  return PMF_OK;
}

int cur_csr_sqnorms(pmf_ctx* c, double* row_sq, double* col_sq) {
  DevTemps tmp;
  double* out = nullptr;
  PMFCHK(cur_csr_sqnorms_f64(c, tmp, true, &out));
  std::vector<double> rows((size_t)c->m);
  HIPCHK(c, hipMemcpyAsync(rows.data(), out, (size_t)c->m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (col_sq) HIPCHK(c, hipMemcpyAsync(col_sq, out + c->mp, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));         // the temporaries are released on return
  if (row_sq) std::memcpy(row_sq, rows.data(), rows.size() * sizeof(double));
  return cur_csr_vnorm2(c, rows.data());
}

// The gathers Cg [mp][cp], Rg [rp][np] (within the buffers of cur_alloc) and M [cp][rp] (host) = Cg^T data Rg^T from the stored
// entries: hr, hc the checked indices of the call.  Chunks of PMF_CURSP_CHUNK entries over the longest selected row.
int cur_csr_mid(pmf_ctx* c, const std::vector<int>& hr, const std::vector<int>& hc, int cp, int rp, std::vector<double>& M) {
  const int nr = (int)hr.size(), nc = (int)hc.size(), np = c->np;
  const int64_t mp = c->mp;
  int64_t longest = 0;
  for (int r : hr) longest = std::max(longest, c->cur_ip[(size_t)r + 1] - c->cur_ip[(size_t)r]);
  const int64_t nchunks = std::max<int64_t>(1, (longest + PMF_CURSP_CHUNK - 1) / PMF_CURSP_CHUNK);
  if (nchunks > 65535) return fail(c, PMF_EINVAL, "pmf_cur_compute: a selected row of more than 16 776 960 stored entries is not supported by this build");
  DevTemps tmp;
  int *dcid = nullptr, *drid = nullptr;
  double *part = nullptr, *dM = nullptr;
  PMFCHK(talloc(c, tmp, &dcid, (size_t)nc));
  PMFCHK(talloc(c, tmp, &drid, (size_t)rp));          // (slots >= nr: row 0, an index in range; their sums are not read)
  PMFCHK(talloc(c, tmp, &part, (size_t)nchunks * rp * cp));
  PMFCHK(talloc(c, tmp, &dM, (size_t)cp * rp));
  HIPCHK(c, hipMemcpyAsync(dcid, hc.data(), (size_t)nc * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(drid, hr.data(), (size_t)nr * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->dCurCg, 0, (size_t)mp * cp * sizeof(float), c->stream));
  HIPCHK(c, hipMemsetAsync(c->dCurRg, 0, (size_t)rp * np * sizeof(float), c->stream));
  hipLaunchKernelGGL(k_cur_csr_gather, dim3((unsigned)(nc + nr)), dim3(256), 0, c->stream, (const int64_t*)c->dIndptr, (const int32_t*)c->dIndices,
                     (const float*)c->dVals, (const int64_t*)c->dTIndptr, (const int32_t*)c->dTIndices, (const float*)c->dTVals,
                     (const int*)dcid, nc, cp, (const int*)drid, np, c->dCurCg, c->dCurRg);
  HIPCHK(c, hipGetLastError());
  if (c->profile && c->stat.site == SITE_CUR) {
    c->stat.name = cp == 64 ? "k_cur_csr_mid<1>" : "k_cur_csr_mid<2>";
    // expected crossings: the entries of the selected rows times the mean column length; a product and two sums for each of the cp lanes
    const double cross = (double)nr * ((double)c->nnz / (double)c->m) * ((double)c->nnz / (double)c->n);
    c->stat.flops = c->stat.exec_flops = 2.0 * cross * cp;
    c->stat.bytes = cross * (8.0 + 4.0 * cp);          // an entry of the column and a row of Cg per crossing (Cg from L2)
  }
  const dim3 grid((unsigned)nr, (unsigned)nchunks);
  stat_begin(c, SITE_CUR);
  if (cp == 64)
    hipLaunchKernelGGL(k_cur_csr_mid<1>, grid, dim3(256), 0, c->stream, (const int64_t*)c->dIndptr, (const int32_t*)c->dIndices, (const float*)c->dVals,
                       (const int64_t*)c->dTIndptr, (const int32_t*)c->dTIndices, (const float*)c->dTVals, (const int*)drid, (const float*)c->dCurCg, rp, part);
  else
    hipLaunchKernelGGL(k_cur_csr_mid<2>, grid, dim3(256), 0, c->stream, (const int64_t*)c->dIndptr, (const int32_t*)c->dIndices, (const float*)c->dVals,
                       (const int64_t*)c->dTIndptr, (const int32_t*)c->dTIndices, (const float*)c->dTVals, (const int*)drid, (const float*)c->dCurCg, rp, part);
  stat_end(c, SITE_CUR);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_cur_csr_mid_reduce, dim3((unsigned)((cp * rp + 255) / 256)), dim3(256), 0, c->stream, (const double*)part, (int)nchunks, cp, rp, dM);
  HIPCHK(c, hipGetLastError());
  M.resize((size_t)cp * rp);
  HIPCHK(c, hipMemcpyAsync(M.data(), dM, M.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));         // the temporaries are released on return
  return PMF_OK;
}

// A [q][q] (host) = dd^T o the float64 Gram matrix of the gathered G (cur_gram_pinv's operand)
int cur_csr_gram(pmf_ctx* c, const float* G, int64_t ldg, int q, int qp, int inner, bool trans, const std::vector<double>& d, std::vector<double>& A) {
  DevTemps tmp;
  double* dA = nullptr;
  PMFCHK(talloc(c, tmp, &dA, (size_t)qp * qp));
  PMFCHK(gram_f64(c, G, ldg, qp, inner, trans, dA, tmp));
  std::vector<double> full((size_t)qp * qp);
  HIPCHK(c, hipMemcpyAsync(full.data(), dA, full.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));         // the temporaries are released on return
  A.resize((size_t)q * q);
  for (int i = 0; i < q; ++i)
    for (int j = 0; j < q; ++j) A[(size_t)i * q + j] = full[(size_t)i * qp + j] * (d[(size_t)i] * d[(size_t)j]);
  return PMF_OK;
}

// ||data - C U R||^2 = ||data||^2 - 2 <U, Mt> + <(C^T C) U, U (R R^T)> with Mt = C^T data R^T = dc o M o dr: float64, a fixed
// order, clamped at 0 before the root.  No pass over a dense image.
int cur_csr_ferr(pmf_ctx* c, const std::vector<double>& M, int rp, const std::vector<double>& dc, const std::vector<double>& dr,
                 const std::vector<double>& U) {
  const int nc = (int)dc.size(), nr = (int)dr.size(), cp = (int)round_up(nc, 64);
  PMFCHK(cur_csr_vnorm2(c, nullptr));
  std::vector<double> GC, GR;
  PMFCHK(cur_csr_gram(c, c->dCurCg, cp, nc, cp, (int)c->mp, true, dc, GC));
  PMFCHK(cur_csr_gram(c, c->dCurRg, c->np, nr, rp, c->np, false, dr, GR));
  double cross = 0.0, quad = 0.0;
  for (int a = 0; a < nc; ++a)
    for (int b = 0; b < nr; ++b) cross += U[(size_t)a * nr + b] * (dc[(size_t)a] * M[(size_t)a * rp + b] * dr[(size_t)b]);
  std::vector<double> X((size_t)nc * nr, 0.0), Y((size_t)nc * nr, 0.0);     // X = (C^T C) U, Y = U (R R^T)
  for (int a = 0; a < nc; ++a)
    for (int q = 0; q < nc; ++q) {
      const double g = GC[(size_t)a * nc + q];
      for (int b = 0; b < nr; ++b) X[(size_t)a * nr + b] += g * U[(size_t)q * nr + b];
    }
  for (int a = 0; a < nc; ++a)
    for (int q = 0; q < nr; ++q) {
      const double u = U[(size_t)a * nr + q];
      for (int b = 0; b < nr; ++b) Y[(size_t)a * nr + b] += u * GR[(size_t)q * nr + b];
    }
  for (size_t e = 0; e < X.size(); ++e) quad += X[e] * Y[e];
  const double f2 = c->cur_vnorm2 - 2.0 * cross + quad;
  c->cur_ferr = std::sqrt(f2 > 0.0 ? f2 : 0.0);
  c->cur_ferr_valid = true;
  return PMF_OK;
}

int cur_ferr(pmf_ctx* c, double* out) {
  if (!cur_csr(c)) return fail(c, PMF_EINVAL, "pmf_cur_ferr: CSR data only (pmf_frobenius is the error on dense data)");
  if (!c->cur_valid || !c->cur_ferr_valid) return fail(c, PMF_EINVAL, "pmf_cur_ferr: no decomposition of the current data (pmf_cur_compute first)");
  *out = c->cur_ferr;
  return PMF_OK;
}

}  // namespace
