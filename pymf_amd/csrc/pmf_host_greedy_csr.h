// pmf_host_greedy_csr.h -- GREEDY on CSR data: the checked upload with its transposed copy, the rounds of the wide case over stored
// entries, the gather of W, H^T = V^T pinv(W)^T and the error by the trace identity (kernels: pmf_greedy_csr.h, pmf_greedy.h,
// pmf_svd_csr.h, pmf_cur_csr.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
//
// State (pmf_ctx): v_csr on a GREEDY context = both CSR images resident (dIndptr ... of V, dTIndptr ... of V^T) and no dense V: dV
// is released by the upload, so every dense-only entry point finds no data.  The Gram matrix and its eigenpairs are the dense
// path's buffers (dGrG, dGrQT, gr_ev, gr_ord), the selection is dSvSel, W is dW (float32: bit-exact columns of the data).  H lives
// as H^T [np][64] float64 in dGrHTd while gr_ht_valid; dH holds an H that the caller uploaded (gr_ht_valid off) and is not
// written by the H step.
#pragma once

namespace {

bool greedy_csr(const pmf_ctx* c) { return c->algo == PMF_ALGO_GREEDY && c->v_csr; }

// the entry points that have no CSR form on a GREEDY context
int greedy_csr_refuse(pmf_ctx* c, const char* who) {
  if (!c || !greedy_csr(c)) return PMF_OK;
  return fail(c, PMF_EINVAL, std::string(who) + ": not while CSR data is resident on a GREEDY context (pmf_update_w, pmf_update_h, pmf_factorize, "
                                                "pmf_frobenius, pmf_greedy_select, pmf_sivm_get_select and the factor transfers work on it; "
                                                "dense data brings the rest back)");
}

int greedy_csr_ht(pmf_ctx* c, bool to_h) {
  const int64_t elems = (int64_t)c->np * PMF_GCSR_LD;
  hipLaunchKernelGGL(k_greedy_csr_ht, dim3(elem_grid(elems)), dim3(256), 0, c->stream, c->dH, c->np, c->k, elems, c->dGrHTd, to_h ? 1 : 0);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// dense data came back to the context: the CSR arrays go, an H that lived in float64 is rounded into dH
int greedy_csr_left(pmf_ctx* c) {
  if (c->algo != PMF_ALGO_GREEDY || !c->dIndptr) return PMF_OK;
  if (c->gr_ht_valid && c->dGrHTd) PMFCHK(greedy_csr_ht(c, true));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dIndptr));
  PMFCHK(dfree(c, &c->dIndices));
  PMFCHK(dfree(c, &c->dVals));
  PMFCHK(dfree(c, &c->dTIndptr));
  PMFCHK(dfree(c, &c->dTIndices));
  PMFCHK(dfree(c, &c->dTVals));
  PMFCHK(dfree(c, &c->dGrHTd));
  PMFCHK(dfree(c, &c->dCslabs));
  c->nnz = 0; c->v_csr = false; c->gr_ht_valid = false;
  c->path = "greedy_panels";
  choose_stat_site(c, false);
  return PMF_OK;
}

// pmf_set_v_csr_f32 on a GREEDY context: refused arrays never reach the device and leave the resident data as it was
int greedy_csr_set_v(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz) {
  if (c->nranks > 1 || multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_set_v_csr_f32: GREEDY on CSR data: one rank only in this build");
  if (std::min<int64_t>(c->mp, c->np) > PMF_GRAM_MAX_NP)
    return fail(c, PMF_EINVAL, "pmf_set_v_csr_f32: GREEDY on CSR data: min(rows, cols) > 1024 is not supported by this build");
  const char* why = csr_check(c->m, c->n, indptr, indices, nnz);
  if (!why) why = csr_check_ascending(c->m, indptr, indices);
  if (why) return fail(c, PMF_EINVAL, std::string("pmf_set_v_csr_f32: ") + why);
  CsrPair p;
  csr_transpose_host(c, indptr, indices, vals, nnz, p);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dV));                            // a CSR upload replaces dense data
  PMFCHK(csr_upload_pair(c, p, indices, vals, nnz));
  c->nnz = nnz; c->have_v = true; c->v_csr = true; c->csr_dense = false;
  v_replaced(c);                                       // (the cached eigenpairs with it)
  c->path = "greedy_csr";
  choose_stat_site(c, false);
  return PMF_OK;
}

// greedy_eig's Gram matrix of the short side from stored entries, exact (k_csr_gram): V^T V from the image of V for rows > cols,
// V V^T from the image of V^T otherwise
int greedy_csr_gram(pmf_ctx* c, bool left, int qp, double* G) {
  return left ? csr_gram_f64(c, c->dIndptr, c->dIndices, c->dVals, c->nnz, c->m, qp, G)
              : csr_gram_f64(c, c->dTIndptr, c->dTIndices, c->dTVals, c->nnz, c->n, qp, G);
}

// The rounds of the wide case on CSR data (greedy_select has staged order, dsv and taken): the candidates are the lines of the image
// of V^T, or of V for the selection on the transposed view -- both are resident, so neither needs a copy.  Enqueued back to back.
int greedy_csr_rounds(pmf_ctx* c, bool trans, int nsel, int cc, const int* order, const double* dsv, unsigned char* taken, int* dsel, DevTemps& tmp) {
  const int R = (int)(trans ? c->n : c->m), C = (int)(trans ? c->m : c->n);
  const int Rp = (int)round_up(R, 64), Cp = (int)round_up(C, 64);
  double* sq = nullptr;
  PMFCHK(cur_csr_sqnorms_f64(c, tmp, false, &sq));
  const double* nrm2 = trans ? sq : sq + c->mp;
  double *Bp = nullptr, *Q = nullptr, *pscore = nullptr;
  float* Op = nullptr;
  int* pidx = nullptr;
  PMFCHK(talloc(c, tmp, &Bp, (size_t)std::max(cc, 1) * Rp));
  PMFCHK(talloc(c, tmp, &Q, (size_t)nsel * Rp));
  PMFCHK(talloc(c, tmp, &Op, (size_t)Rp * PMF_GREEDY_OPW));
  PMFCHK(talloc(c, tmp, &pscore, (size_t)PMF_CL_MAX_WGS));
  PMFCHK(talloc(c, tmp, &pidx, (size_t)PMF_CL_MAX_WGS));
  const int64_t op_elems = (int64_t)Rp * PMF_GREEDY_OPW;
  hipLaunchKernelGGL(k_greedy_init, dim3(elem_grid(std::max<int64_t>(op_elems, Cp))), dim3(256), 0, c->stream, (const double*)c->dGrQT, Rp,
                     order, dsv, cc, R, Rp, 1, Bp, Op, op_elems, (const double*)nullptr, (double*)nullptr, taken, Cp);
  HIPCHK(c, hipGetLastError());
  const int lpw = (int)round_up(std::max<int64_t>(PMF_GCSR_MIN_LINES, (C + PMF_CL_MAX_WGS - 1) / PMF_CL_MAX_WGS), 4);
  const int wgs = (C + lpw - 1) / lpw;
  GreedyCsrPassArgs p{};
  p.indptr = trans ? c->dIndptr : c->dTIndptr;
  p.indices = trans ? c->dIndices : c->dTIndices;
  p.vals = trans ? c->dVals : c->dTVals;
  p.Op = Op; p.nrm2 = nrm2; p.taken = taken; p.pscore = pscore; p.pidx = pidx; p.lines = C; p.lines_per_wg = lpw; p.c = cc;
  GreedyStepArgs s{};
  s.pscore = pscore; s.pidx = pidx; s.nrm2 = nrm2; s.Bp = Bp; s.Q = Q; s.Op = Op; s.select = dsel; s.taken = taken; s.ldb = Rp;
  s.m = R; s.n = C; s.c = cc; s.nparts = wgs;
  s.indptr = p.indptr; s.indices = p.indices; s.vals = p.vals;
  for (int i = 0; i < nsel; ++i) {
    const int cpl = cc + i <= 64 ? 1 : 2;
    if (c->profile && c->stat.site == SITE_GREEDY) {   // the record of the launch at hand
      c->stat.name = cpl == 1 ? "k_greedy_csr_pass<1>" : "k_greedy_csr_pass<2>";
      c->stat.flops = c->stat.exec_flops = 2.0 * (double)c->nnz * (double)(cc + i);
      // the entries, the pointers; the operand's rows (one or two 64-column halves, from L2)
      c->stat.bytes = 12.0 * (double)c->nnz + 8.0 * (double)C + 4.0 * 64.0 * cpl * (double)R;
    }
    stat_begin(c, SITE_GREEDY);
    if (cpl == 1) hipLaunchKernelGGL(k_greedy_csr_pass<1>, dim3((unsigned)wgs), dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL(k_greedy_csr_pass<2>, dim3((unsigned)wgs), dim3(256), 0, c->stream, p);
    stat_end(c, SITE_GREEDY);
    HIPCHK(c, hipGetLastError());
    s.round = i;
    hipLaunchKernelGGL(k_greedy_step_csr, dim3(1), dim3(256), 0, c->stream, s);
    HIPCHK(c, hipGetLastError());
  }
  return PMF_OK;
}

// W = V[:, select] on CSR data: the chosen columns are lines of the image of V^T, scattered into the zeroed dW
int greedy_csr_gather_w(pmf_ctx* c) {
  HIPCHK(c, hipMemsetAsync(c->dW, 0, (size_t)c->mp * c->KP * sizeof(float), c->stream));
  hipLaunchKernelGGL(k_greedy_csr_gather, dim3((unsigned)c->k), dim3(256), 0, c->stream, (const int64_t*)c->dTIndptr, (const int32_t*)c->dTIndices,
                     (const float*)c->dTVals, (const int*)c->dSvSel, c->KP, c->dW);
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  c->sv_have_select = true;
  return PMF_OK;
}

// GREEDY.update_h on CSR data: pinv(W) as on dense data (cur_gram_pinv on dW), then H^T = V^T pinv(W)^T, one k_csr_proj_f64 pass
// over the image of V^T, float64 throughout
int greedy_csr_update_h(pmf_ctx* c) {
  const int k = c->k, KP = c->KP;
  if (!c->dGrHTd) PMFCHK(dalloc(c, &c->dGrHTd, (size_t)c->np * PMF_GCSR_LD));
  std::vector<double> P;
  {
    DevTemps tmp;
    float* Wp = nullptr;                                // W in the 64-column tile of the Gram kernel
    PMFCHK(talloc(c, tmp, &Wp, (size_t)c->mp * 64));
    HIPCHK(c, hipMemcpy2DAsync(Wp, 64 * sizeof(float), c->dW, (size_t)KP * sizeof(float), (size_t)KP * sizeof(float), (size_t)c->mp,
                               hipMemcpyDeviceToDevice, c->stream));
    PMFCHK(cur_gram_pinv(c, Wp, 64, k, 64, (int)c->mp, true, std::vector<double>((size_t)k, 1.0), P));
  }
  DevTemps tmp;
  double *dP = nullptr, *B = nullptr;
  PMFCHK(talloc(c, tmp, &dP, P.size()));
  PMFCHK(talloc(c, tmp, &B, (size_t)c->mp * PMF_GCSR_LD));
  HIPCHK(c, hipMemcpyAsync(dP, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const int64_t elems = c->mp * PMF_GCSR_LD;
  hipLaunchKernelGGL(k_greedy_csr_pinv_t, dim3(elem_grid(elems)), dim3(256), 0, c->stream, (const float*)c->dW, (const double*)dP, c->m, k, KP, elems, B);
  HIPCHK(c, hipGetLastError());
  PMFCHK(svd_csr_proj(c, true, B, PMF_GCSR_LD, PMF_GCSR_LD, c->dGrHTd, PMF_GCSR_LD, false));
  h_replaced(c, false, true);
  c->gr_ht_valid = true;
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  return PMF_OK;
}

// pmf_frobenius / the error behind an iteration on CSR data: the float64 trace identity (svd_csr_err) on a float64 copy of W and
// on H^T; an H from the caller (dH) is widened first
int greedy_csr_error(pmf_ctx* c, double* out) {
  if (!c->dGrHTd) PMFCHK(dalloc(c, &c->dGrHTd, (size_t)c->np * PMF_GCSR_LD));
  if (!c->gr_ht_valid) {
    PMFCHK(greedy_csr_ht(c, false));
    c->gr_ht_valid = true;
  }
  DevTemps tmp;
  double* Wd = nullptr;
  PMFCHK(talloc(c, tmp, &Wd, (size_t)c->mp * PMF_GCSR_LD));
  const int64_t elems = c->mp * PMF_GCSR_LD;
  hipLaunchKernelGGL(k_greedy_csr_widen, dim3(elem_grid(elems)), dim3(256), 0, c->stream, (const float*)c->dW, c->KP, c->k, elems, Wd);
  HIPCHK(c, hipGetLastError());
  return svd_csr_err(c, Wd, c->dGrHTd, PMF_GCSR_LD, PMF_GCSR_LD, out);   // (synchronises: the temporary is released on return)
}

// H [k][n] from H^T on the device
template <typename T>
int greedy_csr_get_h(pmf_ctx* c, T* H) {
  const int k = c->k;
  const int64_t n = c->n;
  std::vector<double> h((size_t)n * PMF_GCSR_LD);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->dGrHTd, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < k; ++i)
    for (int64_t col = 0; col < n; ++col) H[(size_t)i * n + col] = (T)h[(size_t)col * PMF_GCSR_LD + i];
  return PMF_OK;
}

}  // namespace
