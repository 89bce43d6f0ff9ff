// pmf_host_cnmf.h -- CNMF in Gram space with its k-means initialisation (kernels: pmf_cnmf.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// ---- CNMF (pymf/cnmf.py) in Gram space: kernels in pmf_cnmf.h ------------------------------------------------------------
// C = V^T V (ensure_vgram, float64, formed once per V) carries the whole loop: every product of cnmf.py:157-175 is one with
// C, pos(C) or neg(C) and an n x k float64 matrix, or a k x k one.  W = V G is materialised when it is read (materialize_w).
int cnmf_alloc(pmf_ctx* c) {
  if (c->dGT) return PMF_OK;
  const size_t kn = (size_t)c->KP * c->np, kk = (size_t)c->KP * c->KP;
  for (double** p : {&c->dGT, &c->dCnA, &c->dCnB, &c->dCnHn, &c->dCnHp}) PMFCHK(dalloc(c, p, kn));
  for (double** p : {&c->dCnLA, &c->dCnLB}) PMFCHK(dalloc(c, p, kk));
  PMFCHK(dalloc(c, &c->dCnTT, 2));
  PMFCHK(dalloc(c, &c->dKmDmin, (size_t)c->np));
  PMFCHK(dalloc(c, &c->dKmZcz, (size_t)c->KP));
  PMFCHK(dalloc(c, &c->dKmAsg, (size_t)c->np));
  PMFCHK(dalloc(c, &c->dKmCnt, (size_t)c->KP));
  PMFCHK(dalloc(c, &c->dKmSel, (size_t)c->KP));
  if (!c->dHd) { PMFCHK(dalloc(c, &c->dHd, kn)); PMFCHK(dalloc(c, &c->dSd, kk)); c->hd_synced = false; }
  return PMF_OK;
}

// C of the current V and its trace (one read back per new V)
int cnmf_ensure_c(pmf_ctx* c) {
  if (c->c_valid) return PMF_OK;
  c->cn_ab_valid = c->cn_l_valid = false;
  PMFCHK(ensure_vgram(c));
  hipLaunchKernelGGL(k_cnmf_trace, dim3(1), dim3(1024), 0, c->stream, c->dC, c->np, c->dCnTT);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(&c->cn_trc, c->dCnTT, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

// (neg(C) X, pos(C) X) for XT [KP][np]
int cnmf_split(pmf_ctx* c, const double* XT, double* YnT, double* YpT) {
  hipLaunchKernelGGL(k_cnmf_split_gemm, dim3((unsigned)(c->np / 16), (unsigned)(c->KP / 16)), dim3(64), 0, c->stream, XT, c->dC, c->np,
                     YnT, YpT, c->stop_arg);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// A = neg(C) G, B = pos(C) G (cnmf.py:159-160) and L_A = A^T G, L_B = B^T G of the current G
int cnmf_ensure_ab(pmf_ctx* c) {
  if (c->cn_ab_valid) return PMF_OK;
  PMFCHK(cnmf_split(c, c->dGT, c->dCnA, c->dCnB));
  c->cn_ab_valid = true;
  c->cn_l_valid = false;
  return PMF_OK;
}
int cnmf_ensure_l(pmf_ctx* c) {
  PMFCHK(cnmf_ensure_ab(c));
  if (c->cn_l_valid) return PMF_OK;
  hipLaunchKernelGGL(k_cnmf_kxk2, dim3((unsigned)(c->KP / 16), (unsigned)(c->KP / 16), 2), dim3(64), 0, c->stream, c->dCnA, c->dCnB,
                     c->dGT, c->np, c->KP, c->dCnLA, c->dCnLB, c->stop_arg);
  HIPCHK(c, hipGetLastError());
  c->cn_l_valid = true;
  return PMF_OK;
}

// S = H H^T -> dSd (float64 H)
int cnmf_gram_s(pmf_ctx* c) {
  hipLaunchKernelGGL(k_gram<double>, dim3((unsigned)(c->KP / 16), (unsigned)(c->KP / 16)), dim3(256), 0, c->stream, c->dHd,
                     (int64_t)c->np, c->np, c->KP, c->k, 0.0, c->dG, c->dSd);
  HIPCHK(c, hipGetLastError());
  c->g_valid = false;          // (dG now holds the float32 S: no consumer of the NMF Gram matrix runs on a CNMF context)
  return PMF_OK;
}

int cnmf_mul_step(pmf_ctx* c, double* T, float* Tf, const double* P1, const double* P2, const double* L1, const double* L2,
                  const double* X1, const double* X2) {
  const dim3 grid((unsigned)(c->np / 16));
#define PMF_CNMF_STEP(NT_) hipLaunchKernelGGL(k_cnmf_mul_step<NT_>, grid, dim3(64 * NT_), 0, c->stream, T, Tf, c->np, P1, P2, L1, L2, X1, X2, c->stop_arg)
  switch (c->NT) {
    case 1: PMF_CNMF_STEP(1); break;
    case 2: PMF_CNMF_STEP(2); break;
    case 4: PMF_CNMF_STEP(4); break;
    default: PMF_CNMF_STEP(8); break;
  }
#undef PMF_CNMF_STEP
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// One iteration of cnmf.py:157-175.  s_fresh: dSd holds H H^T of the H the iteration ends with.
int cnmf_iteration(pmf_ctx* c, bool cw, bool ch, bool* s_fresh) {
  PMFCHK(cnmf_ensure_l(c));
  *s_fresh = false;
  if (ch) {                    // H <- H * sqrt((B + H^T G^T A)^T / ((A + H^T G^T B)^T + 1e-9))
    PMFCHK(cnmf_mul_step(c, c->dHd, c->dH, c->dCnB, c->dCnA, c->dCnLA, c->dCnLB, c->dHd, c->dHd));
    c->g_valid = false; c->num_valid = false; c->trace_ready = false;
  }
  if (cw) {                    // S = H H^T;  G <- G * sqrt((pos(C) H^T + A S) / (neg(C) H^T + B S + 1e-9));  W = V G
    PMFCHK(cnmf_gram_s(c));
    *s_fresh = true;
    PMFCHK(cnmf_split(c, c->dHd, c->dCnHn, c->dCnHp));
    PMFCHK(cnmf_mul_step(c, c->dGT, nullptr, c->dCnHp, c->dCnHn, c->dSd, c->dSd, c->dCnA, c->dCnB));
    c->cn_ab_valid = c->cn_l_valid = false;
    c->cn_user_w = false;      // cnmf.py:175 rebinds W to data G
    c->w_implicit = true;
    c->ps_valid = false;
  }
  return PMF_OK;
}

// The error terms of ||V - V G H|| into dCnTT (k_cnmf_err_terms): A, B, L_A, L_B of the current G -- which the next iteration's
// H step reads as they are -- and S of the current H
int cnmf_err_terms(pmf_ctx* c, bool s_fresh) {
  PMFCHK(cnmf_ensure_l(c));
  if (!s_fresh) PMFCHK(cnmf_gram_s(c));
  hipLaunchKernelGGL(k_cnmf_err_terms, dim3(1), dim3(1024), 0, c->stream, c->dCnA, c->dCnB, c->dHd, (int64_t)c->KP * c->np,
                     c->dCnLA, c->dCnLB, c->dSd, (int64_t)c->KP * c->KP, c->dCnTT, c->stop_arg);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// ||data - W H|| (nmf.py:100-114) as CNMF.frobenius_norm sees it: W = V G through the trace identity
//   ||V - V G H||^2 = tr(C) - 2 <C G, H^T> + <G^T C G, H H^T>,
// the direct residual where that cancels (below 1e-3 of ||V||^2) or where the caller uploaded W.
int cnmf_error(pmf_ctx* c, bool s_fresh, double* out) {
  if (c->cn_user_w) return frobenius_direct(c, out);
  PMFCHK(cnmf_err_terms(c, s_fresh));
  double tt[2] = {0.0, 0.0};
  HIPCHK(c, hipMemcpyAsync(tt, c->dCnTT, sizeof(tt), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double e2 = c->cn_trc - 2.0 * tt[0] + tt[1];
  if (!(e2 > 1e-3 * c->cn_trc)) return frobenius_direct(c, out);
  *out = std::sqrt(e2);
  return PMF_OK;
}

int cnmf_ready(pmf_ctx* c) {
  if (!c->have_g) return fail(c, PMF_EINVAL, "G has not been set (pmf_set_g_f64 / pmf_cnmf_init)");
  PMFCHK(cnmf_alloc(c));
  PMFCHK(cnmf_ensure_c(c));
  return ensure_hd(c);
}

// pmf_factorize for CNMF: the steps of the loop of cnmf.py:156-187 (pmf_host_loop.h).  With the error on and W = V G the loop
// free-runs; near the cancellation threshold and with a caller's W it goes on iteration by iteration.
struct CnmfLoopSteps {
  bool cw, ch;
  int niter;
  bool s_fresh = false;        // dSd holds H H^T of the H the last iteration ended with
  int iterate(pmf_ctx* c, int) { return cnmf_iteration(c, cw, ch, &s_fresh); }   // cnmf.py:121
  int error(pmf_ctx* c, int, double* out) { return cnmf_error(c, s_fresh, out); }   // cnmf.py:150
  bool may_free_run(const pmf_ctx* c, int i, double f) const { return !c->cn_user_w && niter - (i + 1) >= 2 && f * f > 1e-2 * c->cn_trc; }
  int enqueue(pmf_ctx* c, int i, int j, int, double conv_eps) {
    PMFCHK(cnmf_iteration(c, cw, ch, &s_fresh));
    PMFCHK(cnmf_err_terms(c, s_fresh));
    return launch_conv_check(c, c->dCnTT, 1, c->cn_trc, conv_eps, i + j);
  }
  void rewind(pmf_ctx*, int, int) {}                     // (the validity flags describe G and H, which the no-ops left alone)
  int close(pmf_ctx* c) { return materialize_w(c); }     // W = V G once, the W the reference holds after the loop
};

// One pass of the Gram-space k-means: (C Z)^T = Z^T C, z^T C z, the assignment, the counts and the error of iteration `it`
int kmeans_assign_pass(pmf_ctx* c, int it, double eps) {
  const int np = c->np, KP = c->KP;
  double *ZT = c->dCnHn, *CZT = c->dCnHp;
  hipLaunchKernelGGL((k_dgemm_mfma<false>), dim3((unsigned)(np / 16), (unsigned)(KP / 16)), dim3(64), 0, c->stream, ZT, (int64_t)np,
                     c->dC, (int64_t)np, np, CZT, (int64_t)np, (float*)nullptr, (int64_t)0, (const int*)c->dStop);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_kmeans_zcz, dim3((unsigned)c->k), dim3(256), 0, c->stream, ZT, CZT, np, c->dKmZcz, (const int*)c->dStop);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_kmeans_assign, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, c->dC, CZT, c->dKmZcz, (int)c->n, np,
                     c->k, c->dKmAsg, c->dKmDmin, (const int*)c->dStop);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_kmeans_reduce, dim3(1), dim3(1024), 0, c->stream, c->dKmAsg, c->dKmDmin, (int)c->n, c->k, c->dKmCnt, c->dFerr, it,
                     eps, c->dStop);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

}  // namespace
