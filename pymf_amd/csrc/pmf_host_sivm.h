// pmf_host_sivm.h -- SIVM: the selection passes of update_w and the multiplier search of the simplex-constrained H step (kernels: pmf_sivm.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// Rounds of the multiplier search (one solve_nnqps over all columns each) before the H step gives up: the float64
// restatement of the iteration (tests/sivm_oracle.py: simplex_rounds) needs at most 11 on the cases of tests/sivm_cases.py
// (tests/test_sivm_cases.py holds it to half of this).  The first PMF_SIVM_BLIND_ROUNDS are enqueued without a host read.
constexpr int PMF_SIVM_ROUND_CAP = 48;
constexpr int PMF_SIVM_BLIND_ROUNDS = 8;
constexpr double PMF_SIVM_SUM_TOL = 1e-6;   // |sum x - 1|: eight units in the last place of a float32 one

// contiguous ranges of 64-column panels over at most PMF_CL_MAX_WGS workgroups (the partition of cluster_alloc, without its
// slab limit): k_sivm_pass and k_aa_price
void panel_partition(pmf_ctx* c) {
  const int npanels = c->np / 64;
  const int want = std::min(npanels, PMF_CL_MAX_WGS);
  c->sv_ppw = (npanels + want - 1) / want;
  c->sv_wgs = (npanels + c->sv_ppw - 1) / c->sv_ppw;
}

int sivm_alloc(pmf_ctx* c) {
  if (c->dSvState) return PMF_OK;
  panel_partition(c);
  PMFCHK(dalloc(c, &c->dSvState, (size_t)3 * c->np));
  PMFCHK(dalloc(c, &c->dSvPart, (size_t)2 * PMF_CL_MAX_WGS));
  PMFCHK(dalloc(c, &c->dSvPartIdx, (size_t)2 * PMF_CL_MAX_WGS));
  PMFCHK(dalloc(c, &c->dSvSel, (size_t)c->KP));
  PMFCHK(dalloc(c, &c->dSvScal, 2));
  return PMF_OK;
}

int sivm_launch_pass(pmf_ctx* c, const SivmArgs& a) {
  const dim3 grid((unsigned)c->sv_wgs), block(256);
  const size_t smem = (size_t)c->m * sizeof(float);
  stat_begin(c, SITE_SIVM);
  switch (c->sv_metric) {
    case PMF_SIVM_L2: hipLaunchKernelGGL(k_sivm_pass<PMF_SIVM_L2>, grid, block, smem, c->stream, a); break;
    case PMF_SIVM_L1: hipLaunchKernelGGL(k_sivm_pass<PMF_SIVM_L1>, grid, block, smem, c->stream, a); break;
    default: hipLaunchKernelGGL(k_sivm_pass<PMF_SIVM_COSINE>, grid, block, smem, c->stream, a); break;
  }
  stat_end(c, SITE_SIVM);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// SIVM.update_w (sivm.py:145-201): num_bases + 2 ('fastmap') or num_bases ('origin') launches back to back, the closing
// reduce and the gather; nothing is read by the host in between
int sivm_update_w(pmf_ctx* c) {
  PMFCHK(sivm_alloc(c));
  HIPCHK(c, hipMemsetAsync(c->dSvState, 0, (size_t)3 * c->np * sizeof(double), c->stream));
  const bool origin = c->sv_init == 1;
  SivmArgs a{};
  a.V = c->dV;
  a.dij = c->dSvState; a.dsum = c->dSvState + c->np; a.dsq = c->dSvState + 2 * (int64_t)c->np;
  a.select = c->dSvSel; a.scal = c->dSvScal;
  a.np = c->np; a.m = (int)c->m; a.n = (int)c->n;
  a.npanels = c->np / 64; a.panels_per_wg = c->sv_ppw;
  a.fixed_idx = origin ? -1 : 0;
  int pass = 0;
  auto run = [&](int nprev, int use_fixed, int sel_pos, int take_maxd, int plain, int l) -> int {
    const int out = pass & 1, in = out ^ 1;
    a.pscore_in = c->dSvPart + in * PMF_CL_MAX_WGS; a.pidx_in = c->dSvPartIdx + in * PMF_CL_MAX_WGS;
    a.pscore_out = c->dSvPart + out * PMF_CL_MAX_WGS; a.pidx_out = c->dSvPartIdx + out * PMF_CL_MAX_WGS;
    a.nprev = nprev; a.use_fixed = use_fixed; a.sel_pos = sel_pos; a.take_maxd = take_maxd; a.plain = plain; a.l = l;
    ++pass;
    return sivm_launch_pass(c, a);
  };
  // sivm.py:145-166: three distance passes from column 0 ('fastmap'), or one from the origin
  const int nplain = origin ? 1 : 3;
  for (int p = 0; p < nplain; ++p) PMFCHK(run(p == 0 ? 0 : c->sv_wgs, p == 0, -1, 0, 1, 0));
  // sivm.py:181-193: pass l measures against select[l - 1] (the first: the last plain pass's argmax, or -1) and finds select[l]
  for (int l = 1; l < c->k; ++l) PMFCHK(run(c->sv_wgs, origin && l == 1, l - 1, l == 1, 0, l));
  const int last = (pass - 1) & 1;
  hipLaunchKernelGGL(k_sivm_close, dim3(1), dim3(256), 0, c->stream, (const double*)(c->dSvPart + last * PMF_CL_MAX_WGS),
                     (const int*)(c->dSvPartIdx + last * PMF_CL_MAX_WGS), c->sv_wgs, (int)c->n, c->k - 1, c->k == 1 ? 1 : 0,
                     (origin && c->k == 1) ? 1 : 0, c->dSvSel, c->dSvScal);
  HIPCHK(c, hipGetLastError());
  const int64_t elems = c->mp * c->KP;
  hipLaunchKernelGGL(k_sivm_gather, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, c->stream, (const float*)c->dV, (int64_t)c->np,
                     (int)c->m, (int)c->n, c->k, c->KP, elems, (const int*)c->dSvSel, c->dW);
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  c->sv_have_select = true;
  return PMF_OK;
}

// AA.update_h (aa.py:93-111): one simplex-constrained QP per column, as rounds of non-negative QPs (pmf_sivm.h)
int sivm_update_h(pmf_ctx* c) {
  PMFCHK(ensure_ps(c));                          // dPS = (W^T V | W^T W), float32
  if (!c->dSvF) {
    PMFCHK(dalloc(c, &c->dSvF, (size_t)c->KP * c->np));
    PMFCHK(dalloc(c, &c->dSvLam, (size_t)6 * c->np));
    PMFCHK(dalloc(c, &c->dSvSide, (size_t)c->np));
    PMFCHK(dalloc(c, &c->dSvUnf, (size_t)PMF_SIVM_ROUND_CAP + 2));
  }
  // the Hessian W^T W in float64 from the float32 W: the right-hand sides carry the only float32 rounding of the problem
  hipLaunchKernelGGL(k_sivm_hessian, dim3((unsigned)((c->KP * c->KP + 255) / 256)), dim3(256), 0, c->stream, (const float*)c->dW, (int)c->m,
                     c->k, c->KP, c->dGd);
  HIPCHK(c, hipGetLastError());
  PMFCHK(nnqp_prepare(c, c->stream, nnqp_use_quad(c, c->n)));   // inv(W^T W) in dBinv, its pivots' verdict in dWarm
  int spd = 0;
  HIPCHK(c, hipMemcpyAsync(&spd, c->dWarm, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (spd != 1)
    return fail(c, PMF_EINVAL, "SIVM: W^T W is not positive definite, so H is not unique (duplicate selected columns, or "
                               "num_bases > data_dimension)");
  const int64_t ldp = (int64_t)c->np + c->KP;
  HIPCHK(c, hipMemsetAsync(c->dH, 0, (size_t)c->KP * c->np * sizeof(float), c->stream));
  HIPCHK(c, hipMemsetAsync(c->dSvUnf, 0, ((size_t)PMF_SIVM_ROUND_CAP + 2) * sizeof(int), c->stream));
  SivmLamArgs a{};
  a.PS = c->dPS; a.ldp = ldp; a.F = c->dSvF; a.X = c->dH; a.Gd = c->dGd; a.Binv = c->dBinv; a.st = c->dSvLam; a.side = c->dSvSide;
  a.unfinished = c->dSvUnf; a.np = c->np; a.n = (int)c->n; a.k = c->k; a.KP = c->KP; a.round = 0; a.tol = PMF_SIVM_SUM_TOL;
  const dim3 cgrid((unsigned)((c->np + 255) / 256));
  hipLaunchKernelGGL(k_sivm_lam_init, cgrid, dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  int unfinished = -1;
  for (int round = 1; round <= PMF_SIVM_ROUND_CAP; ++round) {
    PMFCHK(solve_nnqps(c, c->dSvF, c->np, 1, c->dH, c->np, 1, c->n, false, /*prepared=*/true));
    a.round = round;
    hipLaunchKernelGGL(k_sivm_lam_update, cgrid, dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    if (round < PMF_SIVM_BLIND_ROUNDS) continue;
    HIPCHK(c, hipMemcpyAsync(&unfinished, c->dSvUnf + round, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (unfinished == 0) break;
  }
  h_replaced(c, false, true);
  if (unfinished != 0)
    return fail(c, PMF_ENUMERIC, "SIVM: the multiplier search of the H step left " + std::to_string(unfinished) + " columns with |sum(h) - 1| > 1e-6 after " +
                                 std::to_string(PMF_SIVM_ROUND_CAP) + " rounds");
  return PMF_OK;
}

// pmf_factorize for SIVM: one iteration (sivm.py:203-228), no free-running form, the direct residual
struct SivmLoopSteps {
  bool cw, ch;
  int iterate(pmf_ctx* c, int) {
    if (cw) PMFCHK(sivm_update_w(c));
    if (ch) PMFCHK(sivm_update_h(c));
    return PMF_OK;
  }
  int error(pmf_ctx* c, int, double* out) { return frobenius_direct(c, out); }
  bool may_free_run(const pmf_ctx*, int, double) const { return false; }
  int enqueue(pmf_ctx* c, int, int, int, double) { return fail(c, PMF_EINVAL, "SIVM: no free-running loop"); }
  void rewind(pmf_ctx*, int, int) {}
  int close(pmf_ctx*) { return PMF_OK; }
};

}  // namespace
