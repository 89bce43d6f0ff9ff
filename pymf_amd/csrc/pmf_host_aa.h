// pmf_host_aa.h -- AA: W_hat = V pinv(H), the rounds of pricing pass and master step of update_w, the closing step (kernels: pmf_aa.h); the H step is sivm_update_h
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// Rounds (one k_aa_price and one k_aa_master each) before the W step gives up: the float64 restatement of the rounds
// (tests/aa_oracle.py: device_rounds) needs at most 52 on the cases of tests/aa_cases.py (tests/test_aa_cases.py holds it to
// half of this), and a corral of PMF_AA_MAX_CORRAL columns takes at least that many rounds to fill.  The first
// PMF_AA_BLIND_ROUNDS are enqueued without a host read.
constexpr int PMF_AA_ROUND_CAP = 512;
constexpr int PMF_AA_BLIND_ROUNDS = 8;
constexpr double PMF_AA_TAU = 2e-6;     // admission: g_min < beta^T g - tau |R| max(|v_e|, |X|): a few float32 roundings of an m-term sum
constexpr double PMF_AA_RHO = 1e-6;     // |R| <= rho max(|W_hat[:, i]|, |X|): X is W_hat[:, i] to float32 precision
constexpr int PMF_AA_WHAT_CHUNK = 8192; // columns per accumulation chain of the W_hat product
constexpr double PMF_AA_PIV = 1e-10;    // the entering column's pivot against its diagonal entry

int aa_corral_ld(const pmf_ctx* c) { return (int)std::min<int64_t>(c->m + 1, c->n) + 1; }   // one slot beyond the largest affinely independent set: the column under test

int aa_alloc(pmf_ctx* c) {
  if (c->dAaX) return PMF_OK;
  panel_partition(c->np / 64, PMF_CL_MAX_WGS, &c->sv_ppw, &c->sv_wgs);
  const int LD = aa_corral_ld(c);
  const size_t E = (size_t)c->mp * c->KP;
  PMFCHK(dalloc(c, &c->dAaWhat, E));
  PMFCHK(dalloc(c, &c->dAaX, E));
  PMFCHK(dalloc(c, &c->dAaR, E));
  PMFCHK(dalloc(c, &c->dAaScore, (size_t)2 * PMF_CL_MAX_WGS * c->KP));
  PMFCHK(dalloc(c, &c->dAaIdx, (size_t)2 * PMF_CL_MAX_WGS * c->KP));
  PMFCHK(dalloc(c, &c->dAaGram, (size_t)c->k * LD * LD));
  PMFCHK(dalloc(c, &c->dAaSlot, (size_t)c->k * LD));
  PMFCHK(dalloc(c, &c->dAaLam, (size_t)c->k * LD));
  PMFCHK(dalloc(c, &c->dAaFin, (size_t)c->k));
  PMFCHK(dalloc(c, &c->dAaUnf, (size_t)PMF_AA_ROUND_CAP + 2));
  PMFCHK(dalloc(c, &c->dAaFlag, 2));
  PMFCHK(dalloc(c, &c->dAaGinv, (size_t)c->KP * c->KP));
  PMFCHK(dalloc(c, &c->dAaBeta, (size_t)c->k * c->n));
  if (!c->dMT) PMFCHK(dalloc(c, &c->dMT, (size_t)c->KP * c->np));
  return PMF_OK;
}

template <int NT>
int aa_launch_price_t(pmf_ctx* c, const AaPriceArgs& a) {
  stat_begin(c, SITE_AA);
  hipLaunchKernelGGL((k_aa_price<NT>), dim3((unsigned)c->sv_wgs), dim3(256), aa_price_smem<NT>(), c->stream, a);
  stat_end(c, SITE_AA);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}
int aa_launch_price(pmf_ctx* c, const AaPriceArgs& a) {
  switch (c->NT) {
    case 1: return aa_launch_price_t<1>(c, a);
    case 2: return aa_launch_price_t<2>(c, a);
    case 4: return aa_launch_price_t<4>(c, a);
  }
  return fail(c, PMF_EINVAL, "AA: bad NT");
}

// W_hat = V pinv(H) = V (inv(H H^T) H)^T for an H of full row rank (aa.py:126, svd.py:27-45)
int aa_what(pmf_ctx* c) {
  PMFCHK(ensure_gram(c, 1.0));
  HIPCHK(c, hipMemsetAsync(c->dAaFlag, 0, 2 * sizeof(int), c->stream));
  hipLaunchKernelGGL((k_inverse_spd_mfma<4>), dim3(1), dim3(256), 0, c->stream, c->dGd, c->KP, c->k, c->dAaGinv, (const int*)nullptr, c->dAaFlag,
                     c->dAaFlag + 1, (double*)nullptr);
  HIPCHK(c, hipGetLastError());
  // M^T = inv(H H^T) H in float64, rounded once (k_snmf_mt), then W_hat = V M^T on the row product, as SNMF's W step: (V H^T)
  // inv(H H^T) would amplify the float32 rounding of V H^T -- sums of positive terms -- by the condition of H
  hipLaunchKernelGGL(k_snmf_mt<float>, dim3((unsigned)(c->np / 16), (unsigned)(c->KP / 16)), dim3(64), 0, c->stream, c->dH, (int64_t)c->np, c->np, c->KP,
                     c->dAaGinv, c->dMT, (float*)nullptr, (double*)nullptr, (const int*)nullptr);
  HIPCHK(c, hipGetLastError());
  // one accumulation chain of the fp32 MFMA over all columns loses about 1e-6 of the sum at 65 536 columns (pmf_host_products.h:
  // PMF_WIDE_K); W_hat is what the W step is measured against, so its chains stay at PMF_AA_WHAT_CHUNK columns and the chunks'
  // results are added in float32 (round to nearest)
  const int64_t E = c->mp * c->KP;
  for (int k0 = 0; k0 < c->np; k0 += PMF_AA_WHAT_CHUNK) {
    const int kc = std::min(PMF_AA_WHAT_CHUNK, c->np - k0);
    PMFCHK(rowgemm_one<EPI_STORE>(c, c->dV + k0, c->np, kc, c->dMT + k0, c->np, nullptr, nullptr, k0 == 0 ? c->dAaWhat : c->dW1));
    if (k0 > 0) {
      hipLaunchKernelGGL(k_acc_f32, dim3(elem_grid(E / 4)), dim3(256), 0, c->stream, c->dAaWhat, c->dW1, E);
      HIPCHK(c, hipGetLastError());
    }
  }
  int flag[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(flag, c->dAaFlag, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (flag[0] != 0 || flag[1] != 1)
    return fail(c, PMF_EINVAL, "AA: H is rank deficient (a pivot of H H^T fell below 1e-8 of its diagonal entry): W_hat = data pinv(H) is "
                               "formed through inv(H H^T), which needs H of full row rank");
  return PMF_OK;
}

// AA.update_w (aa.py:113-134)
int aa_update_w(pmf_ctx* c) {
  PMFCHK(aa_alloc(c));
  PMFCHK(aa_what(c));
  const int LD = aa_corral_ld(c);
  const int64_t E = c->mp * c->KP;
  hipLaunchKernelGGL(k_aa_init, dim3(elem_grid(std::max<int64_t>(E, (int64_t)c->k * LD))), dim3(256), 0, c->stream, (const float*)c->dAaWhat, c->dAaX,
                     c->dAaR, E, c->dAaSlot, c->dAaLam, c->k * LD, c->dAaFin, c->k);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(c->dAaUnf, 0, ((size_t)PMF_AA_ROUND_CAP + 2) * sizeof(int), c->stream));
  const size_t msmem = aa_master_smem(LD);
  {
    static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
    bool& attr_done = attr_done_dev[pmf_current_device()];
    if (!attr_done) {
      HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_aa_master), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)aa_master_smem(PMF_AA_MAX_CORRAL + 1)));
      attr_done = true;
    }
  }
  AaPriceArgs p{};
  p.V = c->dV; p.R = c->dAaR; p.np = c->np; p.m = (int)c->m; p.n = (int)c->n; p.k = c->k;
  p.npanels = c->np / 64; p.panels_per_wg = c->sv_ppw;
  AaMasterArgs a{};
  a.V = c->dV; a.What = c->dAaWhat; a.X = c->dAaX; a.R = c->dAaR; a.A = c->dAaGram; a.cidx = c->dAaSlot; a.lam = c->dAaLam; a.fin = c->dAaFin;
  a.unfinished = c->dAaUnf; a.np = c->np; a.m = (int)c->m; a.n = (int)c->n; a.k = c->k; a.KP = c->KP; a.nparts = c->sv_wgs; a.LD = LD;
  a.tau = PMF_AA_TAU; a.rho = PMF_AA_RHO; a.piv = PMF_AA_PIV;
  int unfinished = -1;
  c->aa_rounds = 0;
  for (int round = 1; round <= PMF_AA_ROUND_CAP; ++round) {
    const size_t off = (size_t)(round & 1) * PMF_CL_MAX_WGS * c->KP;     // the two partials buffers in turn
    p.pscore = c->dAaScore + off; p.pidx = c->dAaIdx + off;
    PMFCHK(aa_launch_price(c, p));
    a.pscore = p.pscore; a.pidx = p.pidx; a.round = round; a.first = round == 1 ? 1 : 0;
    hipLaunchKernelGGL(k_aa_master, dim3((unsigned)c->k), dim3(256), msmem, c->stream, a);
    HIPCHK(c, hipGetLastError());
    c->aa_rounds = round;
    if (round < PMF_AA_BLIND_ROUNDS) continue;
    HIPCHK(c, hipMemcpyAsync(&unfinished, c->dAaUnf + round, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (unfinished == 0) break;
  }
  // the closing step: W = X, beta scattered from the corrals
  HIPCHK(c, hipMemcpyAsync(c->dW, c->dAaX, (size_t)E * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->dAaBeta, 0, (size_t)c->k * c->n * sizeof(double), c->stream));
  hipLaunchKernelGGL(k_aa_beta, dim3((unsigned)c->k), dim3(256), 0, c->stream, (const int*)c->dAaSlot, (const double*)c->dAaLam, LD, (int)c->n, c->dAaBeta);
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  c->aa_have_beta = true;
  if (unfinished != 0)
    return fail(c, PMF_ENUMERIC, "AA: the W step left " + std::to_string(unfinished) + " bases unfinished after " + std::to_string(PMF_AA_ROUND_CAP) +
                                 " rounds of pricing");
  return PMF_OK;
}

// AA.update_h (aa.py:93-111): the step SIVM inherits
int aa_update_h(pmf_ctx* c) {
  c->g_valid = false;                           // (the step forms W^T W where H H^T was)
  return sivm_update_h(c);
}

}  // namespace
