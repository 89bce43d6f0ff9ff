// pmf_host_greedy.h -- GREEDY / GREEDYCUR: the eigenpairs of the short-side Gram matrix, the rounds of the selection on the data or
// on its transposed view, H = pinv(W) data (kernels: pmf_greedy.h, pmf_svd.h, pmf_cur.h); on CSR data: pmf_host_greedy_csr.h
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// The float64 Gram matrix on the short side of V (V V^T for rows <= cols, V^T V otherwise; dGrG) and its eigenpairs (rows of
// dGrQT; gr_ev, gr_ord: those above svd.py's 1e-8 cut in descending order), once per V: the selection on the data and the one on
// its transposed view (GREEDYCUR) share them.  Synchronises.
int greedy_eig(pmf_ctx* c) {
  if (c->gr_eig_valid) return PMF_OK;
  const bool left = c->m > c->n;
  const int q = (int)(left ? c->n : c->m), qp = left ? c->np : (int)c->mp, nj = q + (q & 1);
  if (!c->dGrG) {
    PMFCHK(dalloc(c, &c->dGrG, (size_t)qp * qp));
    PMFCHK(dalloc(c, &c->dGrQT, (size_t)qp * qp));
  }
  DevTemps tmp;
  double *A = nullptr, *A2 = nullptr, *evals = nullptr;
  int* info = nullptr;
  PMFCHK(talloc(c, tmp, &A, (size_t)qp * qp));
  PMFCHK(talloc(c, tmp, &A2, (size_t)qp * qp));
  PMFCHK(talloc(c, tmp, &evals, (size_t)qp));
  PMFCHK(talloc(c, tmp, &info, 2));
  if (greedy_csr(c)) PMFCHK(greedy_csr_gram(c, left, qp, c->dGrG));
  else PMFCHK(gram_f64(c, c->dV, (int64_t)c->np, qp, left ? (int)c->mp : c->np, left, c->dGrG, tmp));
  HIPCHK(c, hipMemcpyAsync(A, c->dGrG, (size_t)qp * qp * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->dGrQT, 0, (size_t)qp * qp * sizeof(double), c->stream));
  PMFCHK(jacobi_eigh_dev(c, A, A2, c->dGrQT, qp, nj, evals, info));
  c->gr_ev.assign((size_t)nj, 0.0);
  HIPCHK(c, hipMemcpyAsync(c->gr_ev.data(), evals, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  c->gr_ord.clear();
  for (int j = 0; j < nj; ++j)
    if (c->gr_ev[(size_t)j] > 1e-8) c->gr_ord.push_back(j);
  std::stable_sort(c->gr_ord.begin(), c->gr_ord.end(), [&](int a, int b) { return c->gr_ev[(size_t)a] > c->gr_ev[(size_t)b]; });
  c->gr_eig_valid = true;
  return PMF_OK;
}

template <int NT>
int greedy_launch_pass_t(pmf_ctx* c, const GreedyPassArgs& a, int wgs) {
  if constexpr (greedy_pass_smem<NT>() > 64 * 1024) {
    static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
    bool& attr_done = attr_done_dev[pmf_current_device()];
    if (!attr_done) {
      HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_greedy_pass<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)greedy_pass_smem<NT>()));
      attr_done = true;
    }
  }
  stat_begin(c, SITE_GREEDY);
  hipLaunchKernelGGL((k_greedy_pass<NT>), dim3((unsigned)wgs), dim3(256), greedy_pass_smem<NT>(), c->stream, a);
  stat_end(c, SITE_GREEDY);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}
// the pass over the first `cols_in_use` columns of the staged operand
int greedy_launch_pass(pmf_ctx* c, const GreedyPassArgs& a, int wgs, int cols_in_use) {
  switch (std::max(1, (cols_in_use + 15) / 16)) {
    case 1: return greedy_launch_pass_t<1>(c, a, wgs);
    case 2: return greedy_launch_pass_t<2>(c, a, wgs);
    case 3: return greedy_launch_pass_t<3>(c, a, wgs);
    case 4: return greedy_launch_pass_t<4>(c, a, wgs);
    case 5: return greedy_launch_pass_t<5>(c, a, wgs);
    case 6: return greedy_launch_pass_t<6>(c, a, wgs);
    case 7: return greedy_launch_pass_t<7>(c, a, wgs);
    case 8: return greedy_launch_pass_t<8>(c, a, wgs);
  }
  return fail(c, PMF_EINVAL, "GREEDY: the staged operand is wider than 128 columns");
}

// greedy.py:105-158 on the resident V, dense or (GREEDY contexts) CSR (trans: on its transposed view, the rows of V being the columns to choose
// from): nsel indices in selection order into dsel (device).  All rounds are enqueued back to back; synchronises at the end.
int greedy_select(pmf_ctx* c, bool trans, int nsel, int* dsel) {
  const bool csr = greedy_csr(c);
  if (!csr && (c->v_csr || !c->dV)) return fail(c, PMF_EINVAL, "GREEDY: dense resident data only");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "GREEDY: one rank only in this build");
  if (nsel < 1 || nsel > PMF_GREEDY_MAX_BASES) return fail(c, PMF_EINVAL, "GREEDY: 1 <= num_bases <= 64");
  if (std::min<int64_t>(c->m, c->n) > PMF_SVD_MAX_RANK) return fail(c, PMF_EINVAL, "GREEDY: min(rows, cols) > 2432 is not supported by this build");
  PMFCHK(greedy_eig(c));
  const bool left = c->m > c->n;
  const bool wide = trans == left;                     // the Gram matrix at hand is A A^T: the pass over column panels of A
  const int qp = left ? c->np : (int)c->mp;
  const int R = (int)(trans ? c->n : c->m), C = (int)(trans ? c->m : c->n);
  const int Rp = (int)round_up(R, 64), Cp = (int)round_up(C, 64);
  const int cc = std::min<int>(nsel, (int)c->gr_ord.size());
  std::vector<double> sv((size_t)std::max(cc, 1), 0.0);
  for (int i = 0; i < cc; ++i) sv[(size_t)i] = std::sqrt(c->gr_ev[(size_t)c->gr_ord[(size_t)i]]);
  DevTemps tmp;
  int* order = nullptr;
  double* dsv = nullptr;
  unsigned char* taken = nullptr;
  PMFCHK(talloc(c, tmp, &order, (size_t)PMF_GREEDY_MAX_BASES));
  PMFCHK(talloc(c, tmp, &dsv, (size_t)PMF_GREEDY_MAX_BASES));
  PMFCHK(talloc(c, tmp, &taken, (size_t)Cp));
  if (cc > 0) {
    HIPCHK(c, hipMemcpyAsync(order, c->gr_ord.data(), (size_t)cc * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dsv, sv.data(), (size_t)cc * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if (!wide) {                                         // Gram space: C == the short side, G = A^T A is dGrG
    double *Cm = nullptr, *d = nullptr, *Wm = nullptr;
    PMFCHK(talloc(c, tmp, &Cm, (size_t)std::max(cc, 1) * qp));
    PMFCHK(talloc(c, tmp, &d, (size_t)qp));
    PMFCHK(talloc(c, tmp, &Wm, (size_t)nsel * qp));
    hipLaunchKernelGGL(k_greedy_init, dim3(elem_grid((int64_t)std::max(cc, 1) * qp)), dim3(256), 0, c->stream, (const double*)c->dGrQT, qp,
                       (const int*)order, (const double*)dsv, cc, C, qp, 0, Cm, (float*)nullptr, (int64_t)0, (const double*)c->dGrG, d, taken, qp);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_greedy_gram, dim3(1), dim3(1024), 0, c->stream, (const double*)c->dGrG, qp, C, cc, nsel, Cm, d, Wm, dsel, taken);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));         // the temporaries are released on return
    return PMF_OK;
  }
  if (csr) {                                           // the wide case over stored entries (pmf_host_greedy_csr.h)
    PMFCHK(greedy_csr_rounds(c, trans, nsel, cc, order, dsv, taken, dsel, tmp));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // the temporaries are released on return
    return PMF_OK;
  }
  // ---- the pass over column panels of A (R <= 2432 rows) -------------------------------------------------------------------
  const float* A = c->dV;
  int64_t ld = c->np;
  if (trans) PMFCHK(transposed_view(c, tmp, &A, &ld));
  double* sq = nullptr;                                // |v_j|^2 in float64: the row sums or the column sums of V^2, whichever side the columns of A are
  PMFCHK(sqnorms_f64(c, tmp, false, &sq));
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
  hipLaunchKernelGGL(k_greedy_init, dim3(elem_grid(std::max<int64_t>(op_elems, Cp))), dim3(256), 0, c->stream, (const double*)c->dGrQT, qp,
                     (const int*)order, (const double*)dsv, cc, R, Rp, 1, Bp, Op, op_elems, (const double*)nullptr, (double*)nullptr, taken, Cp);
  HIPCHK(c, hipGetLastError());
  const int npanels = Cp / 64;
  int ppw = 0, wgs = 0;
  panel_partition(npanels, PMF_CL_MAX_WGS, &ppw, &wgs);
  GreedyPassArgs p{};
  p.A = A; p.Op = Op; p.nrm2 = nrm2; p.taken = taken; p.pscore = pscore; p.pidx = pidx; p.ld = ld; p.m = R; p.n = C; p.c = cc;
  p.npanels = npanels; p.panels_per_wg = ppw;
  GreedyStepArgs s{};
  s.A = A; s.pscore = pscore; s.pidx = pidx; s.nrm2 = nrm2; s.Bp = Bp; s.Q = Q; s.Op = Op; s.select = dsel; s.taken = taken; s.ld = ld; s.ldb = Rp;
  s.m = R; s.n = C; s.c = cc; s.nparts = wgs;
  for (int i = 0; i < nsel; ++i) {
    PMFCHK(greedy_launch_pass(c, p, wgs, cc + i));
    s.round = i;
    hipLaunchKernelGGL(k_greedy_step, dim3(1), dim3(256), 0, c->stream, s);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  return PMF_OK;
}

// pmf_greedy_select: the selection alone, on the data or on its transposed view, read back
int greedy_select_host(pmf_ctx* c, bool trans, int nsel, int32_t* select) {
  if (nsel < 1 || nsel > PMF_GREEDY_MAX_BASES) return fail(c, PMF_EINVAL, "pmf_greedy_select: 1 <= nsel <= 64");
  DevTemps tmp;
  int* dsel = nullptr;
  PMFCHK(talloc(c, tmp, &dsel, (size_t)PMF_GREEDY_MAX_BASES));
  PMFCHK(greedy_select(c, trans, nsel, dsel));
  HIPCHK(c, hipMemcpyAsync(select, dsel, (size_t)nsel * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

// GREEDY.update_w (greedy.py:88-170): the selection, then W = V[:, select]
int greedy_update_w(pmf_ctx* c) {
  if (!c->dSvSel) PMFCHK(dalloc(c, &c->dSvSel, (size_t)c->KP));
  PMFCHK(greedy_select(c, false, c->k, c->dSvSel));
  return greedy_csr(c) ? greedy_csr_gather_w(c) : gather_selected_w(c);
}

// GREEDY.update_h (greedy.py:82-86): H = pinv(W) data, pinv(W) = (W^T W)^+ W^T with svd.py's 1e-8 cut on the eigenvalues (float64
// Gram matrix of the float32 W, float64 Jacobi), rounded once; the k x m by m x n product is the W^T V product of the operand
// pinv(W)^T, as SVD projects its other side
int greedy_update_h(pmf_ctx* c) {
  if (greedy_csr(c)) return greedy_csr_update_h(c);
  if (c->v_csr || !c->dV) return fail(c, PMF_EINVAL, "GREEDY: dense resident data only");
  const int k = c->k, KP = c->KP;
  if (!c->dGrMT) PMFCHK(dalloc(c, &c->dGrMT, (size_t)c->mp * KP));
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
  double* dP = nullptr;
  PMFCHK(talloc(c, tmp, &dP, P.size()));
  HIPCHK(c, hipMemcpyAsync(dP, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const int64_t elems = c->mp * KP;
  hipLaunchKernelGGL(k_greedy_pinv_t, dim3(elem_grid(elems)), dim3(256), 0, c->stream, (const float*)c->dW, (const double*)dP, c->m, k, KP, elems,
                     c->dGrMT);
  HIPCHK(c, hipGetLastError());
  float* w = c->dW;                                     // (P | S) of the operand pinv(W)^T: its P block is H
  c->dW = c->dGrMT;
  c->ps_valid = false;
  const int rc = ensure_ps(c);
  c->dW = w;
  c->ps_valid = false;
  PMFCHK(rc);
  HIPCHK(c, hipMemcpy2DAsync(c->dH, (size_t)c->np * sizeof(float), c->dPS, ((size_t)c->np + KP) * sizeof(float), (size_t)c->np * sizeof(float),
                             (size_t)KP, hipMemcpyDeviceToDevice, c->stream));
  h_replaced(c, false, true);
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  return PMF_OK;
}

// pmf_frobenius and the error behind an iteration: the direct residual on dense data, the trace identity on CSR data
int greedy_error(pmf_ctx* c, double* out) { return greedy_csr(c) ? greedy_csr_error(c, out) : frobenius_direct(c, out); }

}  // namespace
