// pmf_host_vq.h -- pmf_vq_columns / pmf_vq_assign: nq <= 128 query vectors against every column of the resident V (kernels: pmf_vq.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// the arguments both entries share, checked before anything is touched
int vq_check(pmf_ctx* c, const char* who, const float* Q, int64_t ldq, int32_t nq, int32_t metric) {
  const std::string w(who);
  if (c->v_csr) return fail(c, PMF_EINVAL, w + ": the context holds CSR data; dense resident data only");
  if (c->v_csc) return fail(c, PMF_EINVAL, w + ": the context holds CSC data; dense resident data only");
  if (c->st_active || !c->have_v || !c->dV)
    return fail(c, PMF_EINVAL, w + ": no dense data is resident (streamed data never is; pmf_set_v_dense_* first)");
  if (nq < 1 || nq > PMF_VQ_MAX_Q) return fail(c, PMF_EINVAL, w + ": 1 <= nq <= 128");
  if (metric != PMF_VQ_L2 && metric != PMF_VQ_L1) return fail(c, PMF_EINVAL, w + ": metric 0 (l2) or 1 (l1)");
  if (!Q || ldq < nq) return fail(c, PMF_EINVAL, w + ": Q is NULL or ldq < nq");
  return PMF_OK;
}

// what pmf_profile_enable times under "profile_vq": the figures of the launch at hand
void vq_stat(pmf_ctx* c, int site, int metric, int nq) {
  if (!c->profile || c->stat.site != site) return;
  const double m = (double)c->m, n = (double)c->n, q = (double)nq;
  if (site == SITE_VQ) {
    c->stat.name = metric == PMF_VQ_L2 ? "k_vq_pass<l2>" : "k_vq_pass<l1>";
    c->stat.flops = c->stat.exec_flops = 3.0 * m * n * q;                     // difference, square or modulus, sum
    c->stat.bytes = 4.0 * m * (double)c->np + 4.0 * m * q;                   // V once (its rereads per tile of 16 queries come from L2), Q once
  } else {
    c->stat.name = "k_vq_argmin_rows";
    c->stat.flops = c->stat.exec_flops = n * q;
    c->stat.bytes = 8.0 * n * q + 4.0 * n;
  }
}

// the sweep: Q [m][nq] (host, leading dimension ldq) against the resident V.  want_all: the distance block [nq][n] in *dall
// (device, a temporary of the call).  The partials of the argmin per query are left in *part, *pidx ([*wgs][*QP]).
int vq_sweep(pmf_ctx* c, DevTemps& tmp, const float* Q, int64_t ldq, int nq, int metric, bool want_all, double** part, int** pidx, int* wgs,
             int* QP, double** dall) {
  const int m = (int)c->m, n = (int)c->n;
  const int qp = (int)round_up(nq, PMF_VQ_TILE);
  std::vector<float> hq((size_t)m * qp, 0.f);          // [m][QP], pad queries zero
  for (int r = 0; r < m; ++r) std::memcpy(hq.data() + (size_t)r * qp, Q + (int64_t)r * ldq, (size_t)nq * sizeof(float));
  float* dQ = nullptr;
  PMFCHK(talloc(c, tmp, &dQ, hq.size()));
  VqArgs a{};
  a.V = c->dV; a.np = c->np; a.m = m; a.n = n;
  a.npanels = c->np / 64;
  panel_partition(a.npanels, PMF_CL_MAX_WGS, &a.panels_per_wg, wgs);
  PMFCHK(talloc(c, tmp, part, (size_t)*wgs * qp));
  PMFCHK(talloc(c, tmp, pidx, (size_t)*wgs * qp));
  *dall = nullptr;
  if (want_all) {                                      // (every entry is written by the pass: no zero fill of up to 1 GiB)
    PMFCHK(dalloc_raw(c, dall, (size_t)nq * n));
    tmp.c = c;
    tmp.p.push_back(*dall);
  }
  HIPCHK(c, hipMemcpyAsync(dQ, hq.data(), hq.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));          // (hq is released on return)
  a.Q = dQ; a.nq = nq; a.QP = qp; a.dall = *dall; a.want_all = want_all ? 1 : 0;
  a.pscore_out = *part; a.pidx_out = *pidx;
  vq_stat(c, SITE_VQ, metric, nq);
  stat_begin(c, SITE_VQ);
  if (metric == PMF_VQ_L2) hipLaunchKernelGGL(k_vq_pass<PMF_VQ_L2>, dim3((unsigned)*wgs), dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL(k_vq_pass<PMF_VQ_L1>, dim3((unsigned)*wgs), dim3(256), 0, c->stream, a);
  stat_end(c, SITE_VQ);
  HIPCHK(c, hipGetLastError());
  *QP = qp;
  return PMF_OK;
}

// pmf_vq_columns: per query the nearest data column
int vq_columns(pmf_ctx* c, const float* Q, int64_t ldq, int nq, int metric, int32_t* idx_out, double* dist_out) {
  DevTemps tmp;
  double *part = nullptr, *dall = nullptr, *dd = nullptr;
  int *pidx = nullptr, *di = nullptr;
  int wgs = 0, QP = 0;
  PMFCHK(vq_sweep(c, tmp, Q, ldq, nq, metric, false, &part, &pidx, &wgs, &QP, &dall));
  PMFCHK(talloc(c, tmp, &di, (size_t)nq));
  PMFCHK(talloc(c, tmp, &dd, (size_t)nq));
  hipLaunchKernelGGL(k_vq_close, dim3((unsigned)nq), dim3(256), 0, c->stream, (const double*)part, (const int*)pidx, wgs, QP, (int)c->n, di, dd);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(idx_out, di, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (dist_out) HIPCHK(c, hipMemcpyAsync(dist_out, dd, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));          // the temporaries are released on return
  return PMF_OK;
}

// pmf_vq_assign: per data column the nearest query, and the distance block
int vq_assign(pmf_ctx* c, const float* Q, int64_t ldq, int nq, int metric, int32_t* idx_out, double* dist_all) {
  DevTemps tmp;
  double *part = nullptr, *dall = nullptr;
  int *pidx = nullptr, *di = nullptr;
  int wgs = 0, QP = 0;
  const int n = (int)c->n;
  PMFCHK(vq_sweep(c, tmp, Q, ldq, nq, metric, true, &part, &pidx, &wgs, &QP, &dall));
  if (idx_out) {
    PMFCHK(talloc(c, tmp, &di, (size_t)n));
    vq_stat(c, SITE_VQ_ARGMIN, metric, nq);
    stat_begin(c, SITE_VQ_ARGMIN);
    hipLaunchKernelGGL(k_vq_argmin_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double*)dall, nq, n, di);
    stat_end(c, SITE_VQ_ARGMIN);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(idx_out, di, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  }
  if (dist_all) HIPCHK(c, hipMemcpyAsync(dist_all, dall, (size_t)nq * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));          // the temporaries are released on return
  return PMF_OK;
}

}  // namespace
