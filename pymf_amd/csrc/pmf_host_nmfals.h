// pmf_host_nmfals.h -- NMFALS: the non-negative QPs of both half steps (kernels: pmf_nnls_api.h); the per-class W / H steps and the error ||V - W H||
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// ---- NMFALS ---------------------------------------------------------------------------------
int nnqp_warm_flag(pmf_ctx* c, hipStream_t s) {   // dWarm[0] = 1 iff the QPs over the current dGd have unique minimisers
  if (!c->dWarm) PMFCHK(dalloc(c, &c->dWarm, 1));
  if (c->k <= 64) {
    // the blocked Gauss-Jordan of k_inverse_spd_mfma meets exactly the pivots of the unpivoted LDL^T, as ratios to the diagonal
    // already (unit-diagonal scaling), dead bases patched out: its `spd_flag` IS the uniqueness test -- 17 us where the
    // one-wave elimination of k_spd_unique (rounds 2-3) took 28; the inverse itself is a by-product nobody reads here
    if (!c->dBinv) PMFCHK(dalloc(c, &c->dBinv, (size_t)2 * c->KP * c->KP));
    hipLaunchKernelGGL((k_inverse_spd_mfma<4>), dim3(1), dim3(256), 0, s, c->dGd, c->KP, c->k, c->dBinv, (const int*)nullptr, (int*)nullptr, c->dWarm,
                       c->dBinv + (size_t)c->KP * c->KP);
  } else {
    if (!c->dInvA) PMFCHK(dalloc(c, &c->dInvA, (size_t)c->KP * c->KP));
    pmf_launch_spd_unique_big(s, c->dGd, c->KP, c->k, c->dInvA, c->dWarm);
  }
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// (a few thousand problems do not fill the chip four to a wave: the H half step of a tall matrix stays on k_nnqp)
bool nnqp_use_quad(const pmf_ctx* c, int64_t nprob) {
  return c->opt_nnqp_quad && c->k <= 64 && (nprob >= 16384 || c->opt_nnqp_quad == 2);
}
// 64 < num_bases <= 128: k_nnqp_wave (pmf_nnls_wave.h) on B = inv(HA), whatever the number of problems
bool nnqp_use_wave(const pmf_ctx* c) { return c->opt_nnqp_wave && c->k > 64 && c->k <= 128; }

// What a half step's QPs need from HA = dGd alone, on stream s: the uniqueness flag and, for k_nnqp_quad,
// B = inv(HA with its dead variables patched out), one k x k sized launch.
int nnqp_prepare(pmf_ctx* c, hipStream_t s, bool quad) {
  if (quad) {
    // the inverse's own pivots are the uniqueness test (k_inverse_spd_mfma's spd_flag): no k_spd_unique launch
    if (!c->dWarm) PMFCHK(dalloc(c, &c->dWarm, 1));
    if (!c->dBinv) PMFCHK(dalloc(c, &c->dBinv, (size_t)2 * c->KP * c->KP));     // B, and HA with dead variables patched out
    // (dead bases are patched out by the inverse kernel itself, which also writes the patched HA: one launch, not two)
    double* Hp = c->dBinv + (size_t)c->KP * c->KP;
    if (c->k <= 64) hipLaunchKernelGGL((k_inverse_spd_mfma<4>), dim3(1), dim3(256), 0, s, c->dGd, c->KP, c->k, c->dBinv, (const int*)nullptr, (int*)nullptr, c->dWarm, Hp);
    else hipLaunchKernelGGL((k_inverse_spd_mfma<8>), dim3(1), dim3(1024), 0, s, c->dGd, c->KP, c->k, c->dBinv, (const int*)nullptr, (int*)nullptr, c->dWarm, Hp);
    HIPCHK(c, hipGetLastError());
    return PMF_OK;
  }
  return nnqp_warm_flag(c, s);
}

// num_bases > 64: k_nnqp_big keeps one inverse image per workgroup in global memory
int nnqp_scratch(pmf_ctx* c, double** out) {
  *out = nullptr;
  if (c->k <= 64) return PMF_OK;
  if (!c->dQp) {
    const int64_t ks = 64 * pmf_nnqp_big_vpl(c->k);
    PMFCHK(dalloc(c, &c->dQp, (size_t)(pmf_nnqp_big_blocks(c->k, std::max<int64_t>(c->m, c->n)) * ks * ks)));
  }
  *out = c->dQp;
  return PMF_OK;
}

// One half step's problems: F(var, prob) = F[var * f_sk + prob * f_sp], X likewise; HA in dGd.  32 < num_bases <= 64 with a
// well-conditioned HA (dWarm, k_spd_unique): k_nnqp_quad on B = inv(HA); otherwise (and as the fallback the flag
// selects on the device, without a host round trip) k_nnqp / k_nnqp_big.  prepared: nnqp_prepare has run already (the
// streamed W tiles: pmf_stream_begin).
int solve_nnqps(pmf_ctx* c, const float* F, int64_t f_sk, int64_t f_sp, float* X, int64_t x_sk, int64_t x_sp, int64_t nprob, bool stat,
                bool prepared = false) {
  const bool quad = nnqp_use_quad(c, nprob), wave = nnqp_use_wave(c);
  if (!prepared) PMFCHK(nnqp_prepare(c, c->stream, quad || wave));
  double* qp = nullptr;
  PMFCHK(nnqp_scratch(c, &qp));
  if (stat) stat_begin(c, SITE_NNQP_W);
  int rc = PMF_OK;
  QuadCtl ctl{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const bool frames = quad && c->opt_nnqp_frame16;
  if (frames) {
    // The 16-slot frame pays when most problems fit it (settled active sets: three waves per SIMD instead of two).  Whether
    // they do is decided ON THE DEVICE from the count the previous half step of this kind left (no host round trip: the
    // loop is enqueued ahead of the GPU).  Counters rotate over the calls and are zeroed by the kernels themselves.
    const int site = stat ? 0 : 1;                   // W / H half step
    if (!c->dNbig) {
      PMFCHK(dalloc(c, &c->dNbig, 10));
      // no history yet: the first half step of either kind goes to the 32-slot frame (from a random start every system is
      // beyond 16 unknowns, and 262 144 problems appending themselves to the list one atomic each is the slowest way to find out)
      for (int st = 0; st < 2; ++st) HIPCHK(c, hipMemsetAsync(c->dNbig + 5 * st + 2, 0x3f, sizeof(int), c->stream));
    }
    PMFCHK(dgrow(c, &c->dDefer, &c->defer_cap, nprob, 1, /*sync=*/true));
    int* base = c->dNbig + 5 * site;
    const int64_t t = c->quad_calls[site]++;
    ctl.dlist = c->dDefer;
    ctl.nbig = base + (int)(t % 3);
    ctl.nbig_prev = base + (int)((t + 2) % 3);
    ctl.nbig_next = base + (int)((t + 1) % 3);
    ctl.dcount = base + 3 + (int)(t & 1);
    ctl.dcount_next = base + 3 + (int)((t + 1) & 1);
    if (stat && c->opt_nnqp_count) {                  // the W half step's live counts (counting instantiations)
      if (!c->dQstat) PMFCHK(dalloc(c, &c->dQstat, 8));
      ctl.stats = c->dQstat;
    }
  }
  if (quad) rc = pmf_launch_nnqp_quad(c->stream, c->KP, c->k, c->dGd, c->dBinv + (size_t)c->KP * c->KP, c->dBinv, F, f_sk, f_sp, X, x_sk, x_sp, nprob, c->dWarm,
                                  frames ? &ctl : nullptr, stat && c->opt_nnqp_count != 0);
  if (wave) {
    PMFCHK(dgrow(c, &c->dY0, &c->y0_cap, nprob, (size_t)c->KP, /*sync=*/true));   // y0 = inv(HA) f of every problem (k_nnqp_y0): [nprob][KP] float64
    rc = pmf_launch_nnqp_wave(c->stream, c->KP, c->k, c->dGd, c->dBinv + (size_t)c->KP * c->KP, c->dBinv, F, f_sk, f_sp, X, x_sk, x_sp, nprob, c->dWarm, c->dY0);
  }
  if (rc == PMF_OK) rc = pmf_launch_nnqp(c->stream, c->KP, c->k, c->dGd, F, f_sk, f_sp, X, x_sk, x_sp, nprob, c->dWarm, qp, (quad || wave) ? 1 : 0);
  if (stat) stat_end(c, SITE_NNQP_W);
  if (rc != PMF_OK) return fail(c, rc, "nnqp launch failed");
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

int als_update_w(pmf_ctx* c) {
  // HA = H H^T (nmfals.py:93), -FA = V H^T (nmfals.py:88), one QP per row (nmfals.py:89-90)
  PMFCHK(ensure_gram(c, 1.0));
  // (The QPs' preparation -- 56 us of single-workgroup k x k kernels that read HA only -- on a second stream beside
  // V H^T was tried: the iteration got 4 % SLOWER, profiles/r03_experiments.md.)
  PMFCHK(rowgemm<EPI_STORE>(c, c->dV, c->np, c->np, c->dH, c->np, nullptr, nullptr, c->dW1));
  return solve_nnqps(c, c->dW1, 1, c->KP, c->dW, 1, c->KP, c->m, true);
}

int als_update_h(pmf_ctx* c) {
  // HA = W^T W (nmfals.py:78), -FA = W^T V (nmfals.py:73), one QP per column (nmfals.py:74-75)
  c->want_hess = c->nb == 1 && !use_csr(c);
  c->gd_is_s = false;
  const int prc = ensure_ps(c);
  c->want_hess = false;
  PMFCHK(prc);
  const int64_t ldp = (int64_t)c->np + c->KP;
  if (!c->gd_is_s) {           // (the sums were cached, or crossed the ranks after the local reduce)
    pmf_launch_hessian_from_ps(c->stream, c->dPS, ldp, c->np, c->KP, c->k, c->dGd);
    HIPCHK(c, hipGetLastError());
  }
  // problems = columns: f[kk] = PS[kk][col] (stride ldp over kk, 1 over problems)
  PMFCHK(solve_nnqps(c, c->dPS, ldp, 1, c->dH, c->np, 1, c->n, false));
  c->g_valid = false; c->g_parts = 0; c->num_valid = false;
  c->ps_valid = true;
  c->trace_ready = false;
  return PMF_OK;
}

int do_update_w(pmf_ctx* c) {
  c->w_implicit = false;        // about to be overwritten (SNMF) -- only SNMF loops leave it set
  c->ps_valid = false;
  c->psd_fresh = false;
  c->trace_ready = false;
  if (nmf_csr(c)) return nmf_csr_update_w(c);
  switch (c->algo) {
    case PMF_ALGO_NMF: return nmf_update_w(c);
    case PMF_ALGO_BNMF: return nmf_update_w(c);
    case PMF_ALGO_RNMF: return nmf_update_w(c);
    case PMF_ALGO_SNMF: return snmf_update_w(c);
    case PMF_ALGO_NMFALS: return als_update_w(c);
  }
  return fail(c, PMF_EINVAL, "bad algo");
}

int do_update_h(pmf_ctx* c) {
  if (nmf_csr(c)) return nmf_csr_update_h(c);
  switch (c->algo) {
    case PMF_ALGO_NMF: return nmf_update_h(c);
    case PMF_ALGO_BNMF: return nmf_update_h(c);
    case PMF_ALGO_RNMF: return nmf_update_h(c);
    case PMF_ALGO_SNMF: return snmf_update_h(c);
    case PMF_ALGO_NMFALS: return als_update_h(c);
  }
  return fail(c, PMF_EINVAL, "bad algo");
}

int frobenius_direct(pmf_ctx* c, double* out) {
  PMFCHK(materialize_w(c));
  if (c->v_csr) return fail(c, PMF_EINVAL, "frobenius on CSR data: the reference returns its -123456 sentinel (nmf.py:109-112)");
  if (c->v_csc) return fail(c, PMF_EINVAL, "frobenius on CSC data: the reference returns its -123456 sentinel (nmf.py:109-112)");
  const int nb = (int)(c->mp / 64);
  PMFCHK(launch_resid(c, false, 0.f));
  hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(256), 0, c->stream, c->dPart, c->resid_parts, c->dScal);
  HIPCHK(c, hipGetLastError());
  PMFCHK(allreduce_sum(c, c->dScal, 1, true));
  double ss = 0.0;
  HIPCHK(c, hipMemcpyAsync(&ss, c->dScal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out = std::sqrt(ss);
  return PMF_OK;
}

// sum(V^2) over this rank's rows -> dScal[6]; enqueued right behind the upload of a dense V, so the
// first error evaluation does not pay a pass over V
int local_vnorm(pmf_ctx* c) {
  const int nb = 1024;
  hipLaunchKernelGGL(k_sumsq, dim3(nb), dim3(256), 0, c->stream, c->dV, (int64_t)c->mp * c->np, c->dPart);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(256), 0, c->stream, c->dPart, nb, c->dScal + 6);
  HIPCHK(c, hipGetLastError());
  c->vnorm_local_valid = true;
  return PMF_OK;
}

int ensure_vnorm(pmf_ctx* c) {
  if (c->vnorm_valid) return PMF_OK;
  if (!c->vnorm_local_valid) PMFCHK(local_vnorm(c));
  HIPCHK(c, hipMemcpyAsync(c->dScal, c->dScal + 6, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  PMFCHK(allreduce_sum(c, c->dScal, 1, true));
  HIPCHK(c, hipMemcpyAsync(&c->vnorm2, c->dScal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->vnorm_valid = true;
  return PMF_OK;
}

// sqrt(sum((V - W H)^2)) (nmf.py:110).  When the partial sums P = W^T V, S = W^T W of the current
// W are at hand (every iteration that ran update_h), the trace identity
// ||V||^2 - 2<P,H> + <S H,H> gives the same number from k x n sized data in float64 -- no third
// pass over V and, across ranks, no extra collective (P, S are already all-reduced).  The identity
// cancels when the fit is nearly exact; below 1e-3 relative residual energy the direct pass runs.
// part[2 b], part[2 b + 1] = this column block's share of <P, H>, <S H, H> (k_trace_terms): from the float32 (P | S) and H, or --
// SNMF with its float64 H -- from Hd, and inside the Gram-space loop from the float64 P, S of the iteration at hand (psd_fresh)
int launch_trace_terms(pmf_ctx* c) {
  const int nb = c->np / 16;
  const int64_t ldp = (int64_t)c->np + c->KP;
  if (h_in_f64(c)) {
    PMFCHK(ensure_hd(c));
    const size_t smem = (size_t)c->KP * 16 * sizeof(double);
    if (c->psd_fresh && c->ps_valid)
      hipLaunchKernelGGL((k_trace_terms<double, double>), dim3(nb), dim3(256), smem, c->stream, (const double*)c->dHd, (int64_t)c->np, c->np, c->KP,
                         (const double*)c->dPd, (int64_t)c->np, (const double*)c->dSd, (int64_t)c->KP, c->dPart);
    else
      hipLaunchKernelGGL((k_trace_terms<double, float>), dim3(nb), dim3(256), smem, c->stream, (const double*)c->dHd, (int64_t)c->np, c->np, c->KP,
                         (const float*)c->dPS, ldp, (const float*)c->dPS + c->np, ldp, c->dPart);
  } else {
    hipLaunchKernelGGL((k_trace_terms<float, float>), dim3(nb), dim3(256), (size_t)c->KP * 16 * sizeof(float), c->stream, (const float*)c->dH,
                       (int64_t)c->np, c->np, c->KP, (const float*)c->dPS, ldp, (const float*)c->dPS + c->np, ldp, c->dPart);
  }
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

int trace_e2(pmf_ctx* c, double* e2_out) {   // needs ps_valid and vnorm_valid
  double t[2] = {0.0, 0.0};
  if (c->trace_ready && c->ps_valid && c->trace_parts > 0) {   // ... as per-workgroup pairs
    double tp[2 * PMF_HGRAM_MAX_WGS];
    HIPCHK(c, hipMemcpyAsync(tp, c->dT1part, (size_t)2 * c->trace_parts * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < c->trace_parts; ++q) { t[0] += tp[2 * q]; t[1] += tp[2 * q + 1]; }
  } else if (c->trace_ready && c->ps_valid) {   // the H-step kernel already produced both terms
    HIPCHK(c, hipMemcpyAsync(t, c->dScal + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  } else {
    const int nb = c->np / 16;
    PMFCHK(launch_trace_terms(c));
    hipLaunchKernelGGL(k_sum_pairs_f64, dim3(1), dim3(256), 0, c->stream, c->dPart, nb, c->dScal);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(t, c->dScal, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *e2_out = c->vnorm2 - 2.0 * t[0] + t[1];
  return PMF_OK;
}

int do_frobenius(pmf_ctx* c, double* out) {
  if (c->nb > 1) {            // num_bases > 128: the residual through the trace identity (no MFMA residual kernel at that width)
    if (c->v_csr) return fail(c, PMF_EINVAL, "frobenius on CSR data: the reference returns its -123456 sentinel (nmf.py:109-112)");
    if (c->algo != PMF_ALGO_RNMF) {       // (RNMF's (P | S) are contractions with D = S - data, not with V)
      PMFCHK(ensure_ps(c));
      PMFCHK(ensure_vnorm(c));
      double e2 = 0.0;
      PMFCHK(trace_e2(c, &e2));
      if (e2 > 1e-3 * c->vnorm2) { *out = std::sqrt(e2); return PMF_OK; }
    }
    // the identity cancels: direct pass (plain FMAs; num_bases > 128 has no MFMA residual kernel)
    PMFCHK(materialize_w(c));
    PMFCHK(resid_bigk(c, false, c->dScal));
    PMFCHK(allreduce_sum(c, c->dScal, 1, true));
    double ss = 0.0;
    HIPCHK(c, hipMemcpyAsync(&ss, c->dScal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = std::sqrt(ss);
    return PMF_OK;
  }
  if (c->v_csr || !c->ps_valid) return frobenius_direct(c, out);
  PMFCHK(ensure_vnorm(c));
  double e2 = 0.0;
  PMFCHK(trace_e2(c, &e2));
  if (!(e2 > 1e-3 * c->vnorm2)) return frobenius_direct(c, out);
  *out = std::sqrt(e2);
  return PMF_OK;
}

}  // namespace
