// pmf_host_cur.h -- CUR / CMD: the sampling norms, computeUCR (cur.py:99-120 for dense data) and its factors (kernels: pmf_cur.h, pmf_svd.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// csr_ok: the entry point has a form on CSR data (pmf_host_cur_csr.h)
int cur_check(pmf_ctx* c, const char* who, bool csr_ok = false) {
  if (csr_ok && cur_csr(c)) { if (!c->dIndptr) return fail(c, PMF_EINVAL, std::string(who) + ": no resident data"); }
  else if (c->v_csr) return cur_csr_refuse(c, who);
  else if (!c->dV) return fail(c, PMF_EINVAL, std::string(who) + ": dense resident data only");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, std::string(who) + ": one rank only in this build");
  return PMF_OK;
}

// the row sums [mp] and, behind them, the column sums [np] of V^2 in float64, one read of V, into a temporary of the call;
// timed: the launch is the one that SITE_CUR_SQNORMS brackets
int sqnorms_f64(pmf_ctx* c, DevTemps& tmp, bool timed, double** sq) {
  const int64_t mp = c->mp, np = c->np;
  const int npanels = (int)((np + PMF_CUR_PANEL - 1) / PMF_CUR_PANEL), nblocks = (int)(mp / 64);
  double *rowpart = nullptr, *colpart = nullptr;
  PMFCHK(talloc(c, tmp, &rowpart, (size_t)npanels * mp));
  PMFCHK(talloc(c, tmp, &colpart, (size_t)nblocks * np));
  PMFCHK(talloc(c, tmp, sq, (size_t)(mp + np)));
  if (timed) stat_begin(c, SITE_CUR_SQNORMS);
  hipLaunchKernelGGL(k_cur_sqnorms, dim3((unsigned)((int64_t)nblocks * npanels)), dim3(256), 0, c->stream, (const float*)c->dV, np, mp, npanels,
                     rowpart, colpart);
  if (timed) stat_end(c, SITE_CUR_SQNORMS);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_cur_sqnorms_reduce, dim3((unsigned)((mp + np) / 64)), dim3(1024), 0, c->stream, (const double*)rowpart, npanels, mp,
                     (const double*)colpart, nblocks, np, *sq);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// cur.py:84-97 without the normalisation: the row sums (m) and column sums (n) of data^2
int cur_sqnorms(pmf_ctx* c, double* row_sq, double* col_sq) {
  PMFCHK(cur_check(c, "pmf_cur_sqnorms", true));
  if (cur_csr(c)) return cur_csr_sqnorms(c, row_sq, col_sq);
  DevTemps tmp;
  double* out = nullptr;
  PMFCHK(sqnorms_f64(c, tmp, true, &out));
  if (row_sq) HIPCHK(c, hipMemcpyAsync(row_sq, out, (size_t)c->m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (col_sq) HIPCHK(c, hipMemcpyAsync(col_sq, out + c->mp, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  return PMF_OK;
}

int greedy_eig(pmf_ctx* c);   // pmf_host_greedy.h, further down the include order

template <bool TRANS, int NT>
void lev_launch_t(pmf_ctx* c, const double* Pm, int qp, int64_t lp, double* lev) {
  hipLaunchKernelGGL((k_lev_f64<TRANS, NT>), dim3((unsigned)((lp + PMF_LEV_PANEL - 1) / PMF_LEV_PANEL)), dim3(256), 0, c->stream,
                     (const float*)c->dV, (int64_t)c->np, Pm, qp, lp, lev);
}
template <bool TRANS>
int lev_launch(pmf_ctx* c, int nt, const double* Pm, int qp, int64_t lp, double* lev) {
  switch (nt) {
    case 1: lev_launch_t<TRANS, 1>(c, Pm, qp, lp, lev); break;
    case 2: lev_launch_t<TRANS, 2>(c, Pm, qp, lp, lev); break;
    case 3: lev_launch_t<TRANS, 3>(c, Pm, qp, lp, lev); break;
    case 4: lev_launch_t<TRANS, 4>(c, Pm, qp, lp, lev); break;
    case 5: lev_launch_t<TRANS, 5>(c, Pm, qp, lp, lev); break;
    case 6: lev_launch_t<TRANS, 6>(c, Pm, qp, lp, lev); break;
    case 7: lev_launch_t<TRANS, 7>(c, Pm, qp, lp, lev); break;
    case 8: lev_launch_t<TRANS, 8>(c, Pm, qp, lp, lev); break;
    default: return fail(c, PMF_EINVAL, "pmf_cur_leverage: more than 128 singular vectors");
  }
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// cursl.py:66-85 without the division by k and the normalisation: row_lev [m] = the squared row norms of the leading
// min(k_rows, rank) left singular vectors, col_lev [n] = the squared column norms of the leading min(k_cols, rank) right singular
// vectors, float64, from the cached eigenpairs of the Gram matrix on the short side (greedy_eig).  The eigenvector side is
// k_lev_eig, the long side one read of V by k_lev_f64 (pmf_lev.h).  Either pointer may be null.
int cur_leverage(pmf_ctx* c, int k_rows, int k_cols, double* row_lev, double* col_lev) {
  PMFCHK(cur_check(c, "pmf_cur_leverage"));
  if (k_rows < 1 || k_cols < 1) return fail(c, PMF_EINVAL, "pmf_cur_leverage: k_rows, k_cols >= 1");
  if (std::min<int64_t>(c->m, c->n) > PMF_SVD_MAX_RANK) return fail(c, PMF_EINVAL, "pmf_cur_leverage: min(rows, cols) > 2432 is not supported by this build");
  PMFCHK(greedy_eig(c));
  const bool left = c->m > c->n;                        // the eigenvectors are the right singular vectors: the columns' side
  const int rank = (int)c->gr_ord.size();
  const int q = (int)(left ? c->n : c->m), qp = left ? c->np : (int)c->mp;
  const int64_t lp = left ? c->mp : (int64_t)c->np;
  double* out_long = left ? row_lev : col_lev;
  double* out_eig = left ? col_lev : row_lev;
  const int64_t n_long = left ? c->m : c->n;
  // (a side that is not asked for takes no vectors: nothing is checked, sized or launched for it)
  const int kk_long = out_long ? std::min(left ? k_rows : k_cols, rank) : 0, kk_eig = out_eig ? std::min(left ? k_cols : k_rows, rank) : 0;
  if (kk_long > PMF_LEV_MAX_K || kk_eig > PMF_LEV_MAX_K)
    return fail(c, PMF_EINVAL, "pmf_cur_leverage: min(k, rank) > 128 is not supported by this build");
  const int kmax = std::max(std::max(kk_long, kk_eig), 1), nt = std::max(1, (kk_long + 15) / 16);
  std::vector<double> sv((size_t)kmax, 1.0);
  for (int l = 0; l < std::min(kmax, rank); ++l) sv[(size_t)l] = std::sqrt(c->gr_ev[(size_t)c->gr_ord[(size_t)l]]);
  DevTemps tmp;
  int* order = nullptr;
  double *dsv = nullptr, *Pm = nullptr, *lev = nullptr;
  const int64_t pm_elems = kk_long > 0 ? (int64_t)(qp / 64) * nt * 1024 : 0;
  PMFCHK(talloc(c, tmp, &order, (size_t)kmax));
  PMFCHK(talloc(c, tmp, &dsv, (size_t)kmax));
  if (pm_elems > 0) PMFCHK(talloc(c, tmp, &Pm, (size_t)pm_elems));
  PMFCHK(talloc(c, tmp, &lev, (size_t)(lp + qp)));       // the long side, then the eigenvector side (zero filled: kk = 0 leaves zeros)
  if (rank > 0) {
    HIPCHK(c, hipMemcpyAsync(order, c->gr_ord.data(), (size_t)std::min(kmax, rank) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dsv, sv.data(), (size_t)kmax * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if (kk_long > 0) {
    if (left) hipLaunchKernelGGL(k_lev_gather<false>, dim3(elem_grid(pm_elems)), dim3(256), 0, c->stream, (const double*)c->dGrQT, qp, q, kk_long, nt,
                                 (const int*)order, (const double*)dsv, pm_elems, Pm);
    else hipLaunchKernelGGL(k_lev_gather<true>, dim3(elem_grid(pm_elems)), dim3(256), 0, c->stream, (const double*)c->dGrQT, qp, q, kk_long, nt,
                            (const int*)order, (const double*)dsv, pm_elems, Pm);
    HIPCHK(c, hipGetLastError());
    if (c->profile && c->stat.site == SITE_CUR_LEV) {       // the record of the launch at hand (choose_stat_site only names the site)
      char buf[48];
      snprintf(buf, sizeof(buf), "k_lev_f64<%s,%d>", left ? "false" : "true", nt);
      c->stat.name = buf;
      c->stat.flops = 2.0 * (double)c->m * (double)c->n * kk_long;
      c->stat.exec_flops = 2.0 * (double)c->mp * (double)c->np * (16.0 * nt);
      c->stat.bytes = 4.0 * (double)c->mp * (double)c->np + 8.0 * (double)lp;     // V once, one double per position (P from L2)
    }
    stat_begin(c, SITE_CUR_LEV);
    const int rc = left ? lev_launch<false>(c, nt, Pm, qp, lp, lev) : lev_launch<true>(c, nt, Pm, qp, lp, lev);
    stat_end(c, SITE_CUR_LEV);
    PMFCHK(rc);
  }
  if (kk_eig > 0) {
    hipLaunchKernelGGL(k_lev_eig, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->dGrQT, qp, q, kk_eig,
                       (const int*)order, lev + lp);
    HIPCHK(c, hipGetLastError());
  }
  if (out_long) HIPCHK(c, hipMemcpyAsync(out_long, lev, (size_t)n_long * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (out_eig) HIPCHK(c, hipMemcpyAsync(out_eig, lev + lp, (size_t)q * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  return PMF_OK;
}

// P [q][q] (host, row-major) = the pseudo-inverse of diag(d) X diag(d), X = the Gram matrix of the float32 G on the device
// (G [inner][qp], trans; or G [qp][inner]): float64 Gram matrix, scaled, float64 Jacobi, eigenvalues <= 1e-8 dropped
// (svd.py:116-117,141-142 as pinv sees them, svd.py:27-45), the rest taken in descending order: P = sum_j e_j e_j^T / lambda_j
int cur_gram_pinv(pmf_ctx* c, const float* G, int64_t ldg, int q, int qp, int inner, bool trans, const std::vector<double>& d,
                  std::vector<double>& P) {
  DevTemps tmp;
  double *QT = nullptr, *dd = nullptr;
  PMFCHK(talloc(c, tmp, &dd, (size_t)qp));
  HIPCHK(c, hipMemcpyAsync(dd, d.data(), (size_t)q * sizeof(double), hipMemcpyHostToDevice, c->stream));
  std::vector<double> ev;
  std::vector<int> ord;
  PMFCHK(gram_eigh(c, G, ldg, q, qp, inner, trans, dd, tmp, ev, ord, &QT));
  std::vector<double> E(ev.size() * qp);
  HIPCHK(c, hipMemcpyAsync(E.data(), QT, E.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  P.assign((size_t)q * q, 0.0);
  for (int j : ord) {
    const double* e = E.data() + (size_t)j * qp;
    const double inv = 1.0 / ev[(size_t)j];
    for (int a = 0; a < q; ++a) {
      const double ea = e[a] * inv;
      for (int b = 0; b < q; ++b) P[(size_t)a * q + b] += ea * e[b];
    }
  }
  return PMF_OK;
}

int cur_alloc(pmf_ctx* c) {
  if (c->dCurCg) return PMF_OK;
  const int64_t wp = round_up(c->k, 64);              // nr, nc <= k
  PMFCHK(dalloc(c, &c->dCurCg, (size_t)(c->mp * wp)));
  PMFCHK(dalloc(c, &c->dCurRg, (size_t)(wp * c->np)));
  return PMF_OK;
}

// index list of the ABI -> the device's: negative indices count from the end (-1 is the last), counts default to 1
int cur_indices(pmf_ctx* c, const int32_t* id, const int32_t* cnt, int n, int64_t extent, std::vector<int>& idx, std::vector<double>& d) {
  idx.resize((size_t)n);
  d.resize((size_t)n);
  for (int q = 0; q < n; ++q) {
    const int64_t v = id[q] < 0 ? (int64_t)id[q] + extent : (int64_t)id[q];
    if (v < 0 || v >= extent) return fail(c, PMF_EINVAL, "pmf_cur_compute: index out of range");
    if (cnt && cnt[q] < 1) return fail(c, PMF_EINVAL, "pmf_cur_compute: a count must be >= 1");
    idx[(size_t)q] = (int)v;
    d[(size_t)q] = std::sqrt((double)(cnt ? cnt[q] : 1));
  }
  return PMF_OK;
}

// cur.py:99-120 on the resident V: C = data[:, cid] diag(sqrt(ccnt)), R = diag(sqrt(rcnt)) data[rid, :],
// U = pinv(C) data pinv(R) = (C^T C)^+ (dc o (Cg^T data Rg^T) o dr) (R R^T)^+ (pmf_cur.h).  The data are read once by k_prod_f64:
// rows <= cols: T [mp][rp] = V Rg^T, then M = Cg^T T; otherwise T' [cp][np] = Cg^T V, then M = T' Rg^T (float64 MFMA, dgemm64).
// The c x r sized rest runs on the host in float64 in a fixed order.  Leaves W = C U and H = R, so that pmf_frobenius is
// ||data - C U R|| (svd.py:92-107).  On CSR data the gathers and M come from the stored entries (cur_csr_mid) and the error from
// the trace identity (cur_csr_ferr, read by pmf_cur_ferr); everything between is shared.
int cur_compute(pmf_ctx* c, const int32_t* rid, const int32_t* rcnt, int nr, const int32_t* cid, const int32_t* ccnt, int nc) {
  PMFCHK(cur_check(c, "pmf_cur_compute", true));
  if (!rid || !cid) return fail(c, PMF_EINVAL, "pmf_cur_compute: rid and cid must not be NULL");
  const int lim = std::min(c->k, PMF_CUR_MAX_RANK);
  if (nr < 1 || nc < 1 || nr > lim || nc > lim)
    return fail(c, PMF_EINVAL, "pmf_cur_compute: 1 <= nr, nc <= min(128, the context's k) rows and columns");
  std::vector<int> hr, hc;
  std::vector<double> dr, dc;
  PMFCHK(cur_indices(c, rid, rcnt, nr, c->m, hr, dr));
  PMFCHK(cur_indices(c, cid, ccnt, nc, c->n, hc, dc));
  c->cur_valid = c->cur_ferr_valid = false;
  PMFCHK(cur_alloc(c));
  const int64_t mp = c->mp;
  const int np = c->np, cp = (int)round_up(nc, 64), rp = (int)round_up(nr, 64), KP = c->KP;
  const bool trans = c->m > c->n;
  std::vector<double> M((size_t)cp * rp);
  if (cur_csr(c)) {
    PMFCHK(cur_csr_mid(c, hr, hc, cp, rp, M));
  } else {
    DevTemps tmp;
    int *dcid = nullptr, *drid = nullptr;
    double *side = nullptr, *T = nullptr, *dM = nullptr;
    PMFCHK(talloc(c, tmp, &dcid, (size_t)nc));
    PMFCHK(talloc(c, tmp, &drid, (size_t)nr));
    PMFCHK(talloc(c, tmp, &side, trans ? (size_t)rp * np : (size_t)cp * mp));       // Rd [rp][np] or CgT [cp][mp]
    PMFCHK(talloc(c, tmp, &T, trans ? (size_t)cp * np : (size_t)mp * rp));
    PMFCHK(talloc(c, tmp, &dM, (size_t)cp * rp));
    HIPCHK(c, hipMemcpyAsync(dcid, hc.data(), (size_t)nc * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(drid, hr.data(), (size_t)nr * sizeof(int), hipMemcpyHostToDevice, c->stream));
    // (the gathers take the leading dimensions of this call: Cg [mp][cp], Rg [rp][np], both within the buffers of cur_alloc)
    hipLaunchKernelGGL(k_cur_gather, dim3(elem_grid(mp * cp + (int64_t)rp * np)), dim3(256), 0, c->stream, (const float*)c->dV, mp, np,
                       (const int*)dcid, nc, cp, (const int*)drid, nr, rp, c->dCurCg, c->dCurRg, trans ? (double*)nullptr : side,
                       trans ? side : (double*)nullptr);
    HIPCHK(c, hipGetLastError());
    if (trans) {
      PMFCHK(prod_f64(c, true, false, c->dCurCg, cp, cp / 64, c->dV, np, np / 64, (int)mp, T, np, SITE_CUR, tmp));
      PMFCHK(dgemm64(c, T, np, side, np, np, dM, rp, cp, rp, true));
    } else {
      PMFCHK(prod_f64(c, false, false, c->dV, np, (int)(mp / 64), c->dCurRg, np, rp / 64, np, T, rp, SITE_CUR, tmp));
      PMFCHK(dgemm64(c, side, mp, T, rp, (int)mp, dM, rp, cp, rp, false));
    }
    HIPCHK(c, hipMemcpyAsync(M.data(), dM, M.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // the temporaries are released at the end of the block
  }
  std::vector<double> Pc, Pr;
  PMFCHK(cur_gram_pinv(c, c->dCurCg, cp, nc, cp, (int)mp, true, dc, Pc));
  PMFCHK(cur_gram_pinv(c, c->dCurRg, np, nr, rp, np, false, dr, Pr));
  // U = Pc (dc o M o dr) Pr
  std::vector<double> X((size_t)nc * nr, 0.0), U((size_t)nc * nr, 0.0), Us((size_t)nc * nr);
  for (int a = 0; a < nc; ++a)
    for (int q = 0; q < nc; ++q) {
      const double p = Pc[(size_t)a * nc + q] * dc[(size_t)q];
      for (int b = 0; b < nr; ++b) X[(size_t)a * nr + b] += p * (M[(size_t)q * rp + b] * dr[(size_t)b]);
    }
  for (int a = 0; a < nc; ++a)
    for (int q = 0; q < nr; ++q) {
      const double x = X[(size_t)a * nr + q];
      for (int b = 0; b < nr; ++b) U[(size_t)a * nr + b] += x * Pr[(size_t)q * nr + b];
    }
  for (int a = 0; a < nc; ++a)
    for (int b = 0; b < nr; ++b) Us[(size_t)a * nr + b] = dc[(size_t)a] * U[(size_t)a * nr + b];
  {
    DevTemps tmp;
    double *dUs = nullptr, *ddr = nullptr;
    PMFCHK(talloc(c, tmp, &dUs, Us.size()));
    PMFCHK(talloc(c, tmp, &ddr, (size_t)nr));
    HIPCHK(c, hipMemcpyAsync(dUs, Us.data(), Us.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(ddr, dr.data(), (size_t)nr * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_cur_factors, dim3(elem_grid(mp * KP + (int64_t)KP * np)), dim3(256), 0, c->stream, (const float*)c->dCurCg, cp, nc,
                       (const double*)dUs, nr, c->m, mp, KP, (const float*)c->dCurRg, np, (const double*)ddr, c->dW, c->dH);
    HIPCHK(c, hipGetLastError());
    w_replaced(c, false);
    h_replaced(c, false, true);
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (cur_csr(c)) PMFCHK(cur_csr_ferr(c, M, rp, dc, dr, U));
  c->cur_nr = nr; c->cur_nc = nc;
  c->cur_dr = dr; c->cur_dc = dc; c->cur_U = U;
  c->cur_valid = true;
  return PMF_OK;
}

// C (rows x nc), U (nc x nr) and R (nr x cols) of the last cur_compute as float64, row-major; any of them may be null
int cur_get(pmf_ctx* c, double* C, double* U, double* R) {
  if (!c->cur_valid) return fail(c, PMF_EINVAL, "pmf_cur_get: no decomposition of the current data (pmf_cur_compute first)");
  const int nr = c->cur_nr, nc = c->cur_nc, cp = (int)round_up(nc, 64);
  const int64_t m = c->m, n = c->n;
  if (U) std::memcpy(U, c->cur_U.data(), (size_t)nc * nr * sizeof(double));
  std::vector<float> Cg, Rg;
  if (C) {
    Cg.resize((size_t)m * cp);
    HIPCHK(c, hipMemcpyAsync(Cg.data(), c->dCurCg, Cg.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  if (R) {
    Rg.resize((size_t)nr * c->np);
    HIPCHK(c, hipMemcpyAsync(Rg.data(), c->dCurRg, Rg.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (C) for (int64_t row = 0; row < m; ++row) for (int j = 0; j < nc; ++j) C[(size_t)row * nc + j] = (double)Cg[(size_t)row * cp + j] * c->cur_dc[(size_t)j];
  if (R) for (int i = 0; i < nr; ++i) for (int64_t col = 0; col < n; ++col) R[(size_t)i * n + col] = c->cur_dr[(size_t)i] * (double)Rg[(size_t)i * c->np + col];
  return PMF_OK;
}

}  // namespace
