// pmf_host_nmf.h -- NMF / BNMF / RNMF: residual, one-pass and two-pass iterations, the forms for more than 128 bases (kernels: pmf_small.h, pmf_tiled.h, pmf_fused_api.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// What a one-pass launch needs to know about the free-running loop around it; hands over (and clears) the
// pending convergence test.
FusedCtl take_fused_ctl(pmf_ctx* c) {
  FusedCtl ctl{};
  ctl.stop = c->stop_arg ? c->dStop : nullptr;
  ctl.conv_iter = -1;
  if (ctl.stop && c->conv_iter >= 0) {
    ctl.tt = c->conv_tt; ctl.ntt = c->conv_ntt; ctl.ferr = c->dFerr;
    ctl.vnorm2 = c->vnorm2; ctl.eps = c->conv_eps; ctl.nsamp = (double)c->n;
    ctl.conv_iter = c->conv_iter;
    c->conv_iter = -1;
  }
  return ctl;
}

// ---- NMF (multiplicative update) ---------------------------------------------------------
// Leaves c->resid_parts float64 partials in c->dPart.
template <int NT, bool RNMF>
int launch_resid_t(pmf_ctx* c, float lamb, const float* V, const float* W, int64_t rows_p) {
  const int ntiles = (int)(rows_p / 64);
  const size_t res_smem = resid_res_smem_bytes<NT>(c->np);
  if (c->opt_resid_resident && res_smem <= 150 * 1024 && ntiles >= 64) {
    // H resident in LDS, persistent workgroups (a fixed count: the partials' grouping must not depend on the part)
    static bool res_attr_dev[PMF_MAX_DEVICES] = {};
    bool& res_attr = res_attr_dev[pmf_current_device()];
    if (!res_attr) {
      HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_resid_res<NT, RNMF>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
      res_attr = true;
    }
    hipLaunchKernelGGL((k_resid_res<NT, RNMF>), dim3((unsigned)std::min(ntiles, 512)), dim3(256), res_smem, c->stream, V,
                       (int64_t)c->np, c->np, W, c->dH, (int64_t)c->np, lamb, c->dD, c->dPart, ntiles);
    HIPCHK(c, hipGetLastError());
    c->resid_parts = std::min(ntiles, 512);
    return PMF_OK;
  }
  const size_t smem = resid_smem_bytes<NT>();
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_resid<NT, RNMF>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    attr_done = true;
  }
  hipLaunchKernelGGL((k_resid<NT, RNMF>), dim3((unsigned)ntiles), dim3(256), smem, c->stream, V,
                     (int64_t)c->np, c->np, W, c->dH, (int64_t)c->np, lamb, c->dD, c->dPart);
  HIPCHK(c, hipGetLastError());
  c->resid_parts = ntiles;
  return PMF_OK;
}

int launch_resid(pmf_ctx* c, bool rnmf, float lamb, const float* V = nullptr, const float* W = nullptr,
                 int64_t rows_p = 0) {
  if (!V) { V = c->dV; W = c->dW; rows_p = c->mp; }
  switch (c->NT) {
    case 1: return rnmf ? launch_resid_t<1, true>(c, lamb, V, W, rows_p) : launch_resid_t<1, false>(c, lamb, V, W, rows_p);
    case 2: return rnmf ? launch_resid_t<2, true>(c, lamb, V, W, rows_p) : launch_resid_t<2, false>(c, lamb, V, W, rows_p);
    case 4: return rnmf ? launch_resid_t<4, true>(c, lamb, V, W, rows_p) : launch_resid_t<4, false>(c, lamb, V, W, rows_p);
    case 8: return rnmf ? launch_resid_t<8, true>(c, lamb, V, W, rows_p) : launch_resid_t<8, false>(c, lamb, V, W, rows_p);
  }
  return fail(c, PMF_EINVAL, "bad NT");
}

// num_bases > 128: sum((V - W H)^2) over this rank's rows -> *dst (device), plain-FMA tiles; rnmf: D = S - V too
int resid_bigk(pmf_ctx* c, bool rnmf, double* dst, const float* V = nullptr, const float* W = nullptr, int64_t rows_p = 0) {
  if (!V) { V = c->dV; W = c->dW; rows_p = c->mp; }      // (a row tile of a streamed pass otherwise)
  const int gx = c->np / 64, gy = (int)(rows_p / 64);
  const int nb2 = gx * gy;
  DevTemps tmp;                       // frees `part` on every exit
  double* part = nullptr;
  PMFCHK(talloc(c, tmp, &part, (size_t)nb2));
  if (rnmf)
    hipLaunchKernelGGL(k_resid_bigk<true>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, c->stream, V, (int64_t)c->np, W,
                       c->KP, c->dH, (int64_t)c->np, part, (float)c->lamb_w, c->dD);
  else
    hipLaunchKernelGGL(k_resid_bigk<false>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, c->stream, V, (int64_t)c->np, W,
                       c->KP, c->dH, (int64_t)c->np, part, 0.f, (float*)nullptr);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(256), 0, c->stream, part, nb2, dst);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the scratch is freed on return
  return PMF_OK;
}

int rnmf_update_s(pmf_ctx* c) {   // rnmf.py:96-98; also leaves sum((V - W H)^2) in c->rnmf_err2
  const int nb = (int)(c->mp / 64);
  const float lamb = (float)c->lamb_w;
  if (c->nb > 1) {
    PMFCHK(resid_bigk(c, true, c->dScal + 4));
  } else {
    PMFCHK(launch_resid(c, true, lamb));
    hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(256), 0, c->stream, c->dPart, c->resid_parts, c->dScal + 4);
  }
  HIPCHK(c, hipGetLastError());
  PMFCHK(allreduce_sum(c, c->dScal + 4, 1, true));
  HIPCHK(c, hipMemcpyAsync(&c->rnmf_err2, c->dScal + 4, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  c->s_valid = true;
  return PMF_OK;
}

// ---- num_bases > 128 (NMF only): the update rules in blocks of 128 bases on the NT = 8 kernels -------
// W step (nmf.py:128-132): Num = V H^T and Den = W (H H^T) block by block into [mp][KP] buffers, then
// one elementwise pass.  (P | S) (nmf.py:122-124 operands): per base block W_b^T V, and W_b^T W by the
// same kernel with W in the place of V.
// X [rows_p][np] (V, D = S - data, or a streamed tile), Wr / W1r / W2r the same rows of W and of the two [.][KP] temporaries
int bigk_update_w_rows(pmf_ctx* c, const float* X, float* Wr, float* W1r, float* W2r, int64_t rows_p, int64_t mvalid) {
  const bool rn = c->algo == PMF_ALGO_RNMF;
  for (int b = 0; b < c->nb; ++b)                            // Den = W G^T, every block from the OLD W
    PMFCHK((launch_rowgemm<8, EPI_STORE>(c, Wr, c->KP, c->KP, c->dG + (size_t)b * 128 * c->KP, c->KP, nullptr, nullptr,
                                         W2r + b * 128, rows_p, mvalid, c->KP)));
  if (c->opt_rowgemm_stream && c->np % 128 == 0 && c->np <= PMF_WIDE_K) {
    // Num = V H_b^T with the update rule as its epilogue: block b of W is rewritten in place (V H^T does not read W)
    const int ntiles = (int)(rows_p / 32);
    const dim3 grid((unsigned)std::min((ntiles + 3) / 4, 512));     // persistent workgroups (k_rowgemm_stream)
    const size_t smem = (size_t)2 * 128 * 64 * sizeof(float);
    for (int b = 0; b < c->nb; ++b) {
      const float* Hb = c->dH + (size_t)b * 128 * c->np;
      float* Wb = Wr + b * 128;
      const float* Db = W2r + b * 128;
      const int kv = std::max(0, std::min(128, c->k - 128 * b));
      if (rn)
        hipLaunchKernelGGL((k_rowgemm_stream<8, 2, EPI_RNMF_W, true>), grid, dim3(256), smem, c->stream, X, (int64_t)c->np, c->np, Hb,
                           (int64_t)c->np, Wb, Db, (float*)nullptr, (int64_t)0, 0.f, mvalid, kv, ntiles, (int64_t)c->KP);
      else if (c->algo == PMF_ALGO_BNMF)
        hipLaunchKernelGGL((k_rowgemm_stream<8, 2, EPI_BNMF_W, true>), grid, dim3(256), smem, c->stream, X, (int64_t)c->np, c->np, Hb,
                           (int64_t)c->np, Wb, Db, (float*)nullptr, (int64_t)0, (float)c->lamb_w, mvalid, kv, ntiles, (int64_t)c->KP);
      else
        hipLaunchKernelGGL((k_rowgemm_stream<8, 2, EPI_NMF_W, true>), grid, dim3(256), smem, c->stream, X, (int64_t)c->np, c->np, Hb,
                           (int64_t)c->np, Wb, Db, (float*)nullptr, (int64_t)0, 0.f, mvalid, kv, ntiles, (int64_t)c->KP);
      HIPCHK(c, hipGetLastError());
    }
    return PMF_OK;
  }
  PMFCHK(rowgemm<EPI_STORE>(c, X, c->np, c->np, c->dH, c->np, nullptr, nullptr, W1r, rows_p, mvalid));   // (all blocks; in chunks of columns when wide)
  const int64_t count = rows_p * c->KP;
  hipLaunchKernelGGL(k_nmf_w_elem, dim3(elem_grid(count)), dim3(256), 0, c->stream, Wr, W1r, W2r, count,
                     c->algo == PMF_ALGO_BNMF ? 1 : rn ? 2 : 0, (float)c->lamb_w, c->KP, mvalid, c->k);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

int bigk_update_w(pmf_ctx* c) {
  PMFCHK(ensure_gram(c, 0.0));
  const bool rn = c->algo == PMF_ALGO_RNMF;      // rnmf.py:109-115: the contraction runs on D = S - data
  if (rn && !c->s_valid) return fail(c, PMF_EINVAL, "RNMF: S does not exist yet (init_h / update_s create it, rnmf.py:94-98)");
  return bigk_update_w_rows(c, rn ? c->dD : c->dV, c->dW, c->dW1, c->dW2, c->mp, c->m);
}

// acc == nullptr: (P | S) of rows [0, rows_p) of X / Wr into dPS; else added (first: stored) to the float64 image acc
int bigk_ps_rows(pmf_ctx* c, const float* Xv, const float* Wr, int64_t rows_p, int rpc, int nch, double* acc, int first) {
  const int64_t ldp = (int64_t)c->np + c->KP;
  for (int b = 0; b < c->nb; ++b) {
    for (int pass = 0; pass < 2; ++pass) {                 // 0: W_b^T V -> P rows,  1: W_b^T W -> S rows
      const float* X = pass == 0 ? Xv : Wr;
      const int xn = pass == 0 ? c->np : c->KP;
      PMFCHK((launch_colgemm<8, false>(c, X, xn, xn, Wr + b * 128, c->KP, rows_p, rpc, nch)));
      const int64_t cnt4 = (int64_t)128 * xn / 4;
      const size_t off = (size_t)b * 128 * ldp + (pass == 0 ? 0 : c->np);
      if (acc)
        hipLaunchKernelGGL((k_reduce_slabs_block<double>), dim3((unsigned)((cnt4 + 63) / 64)), dim3(1024), 0, c->stream, c->dSlab,
                           nch, 128, xn + 128, xn, acc + off, ldp, first ? 0 : 1);
      else
        hipLaunchKernelGGL((k_reduce_slabs_block<float>), dim3((unsigned)((cnt4 + 63) / 64)), dim3(1024), 0, c->stream, c->dSlab,
                           nch, 128, xn + 128, xn, c->dPS + off, ldp, 0);
      HIPCHK(c, hipGetLastError());
    }
  }
  return PMF_OK;
}

int bigk_ps(pmf_ctx* c) {
  return bigk_ps_rows(c, c->algo == PMF_ALGO_RNMF ? c->dD : c->dV, c->dW, c->mp, c->rows_per_chunk, c->nchunks, nullptr, 0);
}

int nmf_update_w(pmf_ctx* c) {
  if (c->nb > 1) return bigk_update_w(c);
  // The single hook on a fused-kernel shape runs the same one-pass kernel: W is updated and, for the
  // price of the second half of the pass, (W^T V | W^T W) of the new W is already there when
  // update_h() follows (it then costs one k x n sized kernel) -- 0.65 ms for the pair at cfg4
  // instead of 1.12 ms as two tiled passes.
  if ((c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_BNMF) && c->fused_wgs > 0 && !c->fixed_h_loop && !use_csr(c))
    return nmf_fused_pass(c);
  PMFCHK(ensure_gram(c, 0.0));
  if (c->algo == PMF_ALGO_RNMF && !c->s_valid)
    return fail(c, PMF_EINVAL, "RNMF: S does not exist yet (init_h / update_s create it, rnmf.py:94-98)");
  if (c->np > PMF_WIDE_K)       // more columns than one accumulation chain should span: V H^T in chunks, the rule element-wise
    return wide_update_w_rows(c, c->algo == PMF_ALGO_RNMF ? c->dD : c->dV, c->dW, c->mp, c->m);
  if (c->algo == PMF_ALGO_RNMF)
    return rowgemm<EPI_RNMF_W>(c, c->dD, c->np, c->np, c->dH, c->np, c->dW, c->dG, nullptr);
  if (c->algo == PMF_ALGO_BNMF)
    return rowgemm<EPI_BNMF_W>(c, c->dV, c->np, c->np, c->dH, c->np, c->dW, c->dG, nullptr);
  if (c->fixed_h_loop) {
    // H is not updated in this loop, so Num = V H^T is the same every iteration: the first one
    // stores it, the others read it back and never touch V (W*G and the epilogue are all that is left)
    if (!c->dW1) PMFCHK(dalloc(c, &c->dW1, (size_t)std::max<int64_t>(c->mp, c->np) * c->KP));
    if (c->num_valid)
      return rowgemm<EPI_NMF_W_CACHED>(c, c->dV, c->np, c->np, c->dH, c->np, c->dW, c->dG, c->dW1);
    PMFCHK(rowgemm<EPI_NMF_W_SAVE>(c, c->dV, c->np, c->np, c->dH, c->np, c->dW, c->dG, c->dW1));
    c->num_valid = true;
    return PMF_OK;
  }
  stat_begin(c, SITE_ROWGEMM_W);
  const int wrc = rowgemm<EPI_NMF_W>(c, c->dV, c->np, c->np, c->dH, c->np, c->dW, c->dG, nullptr);
  stat_end(c, SITE_ROWGEMM_W);
  return wrc;
}

template <int NT, bool BNMF, bool FOLD>
int launch_h_gram_as(pmf_ctx* c) {
  constexpr size_t smem = hgram_smem_bytes<NT>();
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nmf_h_gram<NT, BNMF, FOLD>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    attr_done = true;
  }
  const int wgs = std::min(c->np / 64, PMF_HGRAM_MAX_WGS);
  // inside pmf_factorize's fused loop the next reader of G is the fused kernel, which adds the
  // per-workgroup partials itself: the kernel then ends without waiting for its last workgroup
  const int final_sum = c->gram_partial_ok ? 0 : 1;
  hipLaunchKernelGGL((k_nmf_h_gram<NT, BNMF, FOLD>), dim3((unsigned)wgs), dim3(1024), smem, c->stream, c->dH, c->np, c->dPS,
                     c->dG, (double*)nullptr /* no reader of the float64 copy on the NMF/BNMF paths */, BNMF ? (float)c->lamb_h : 0.f, c->want_trace ? c->dScal + 2 : nullptr,
                     c->dGpart, c->dT1part, c->dTicket, c->stop_arg, final_sum,
                     FOLD ? c->ipc : IpcPeers{}, c->fold_seq, c->fold_flags, c->dIpcErr, c->ipc_wait_ticks,
                     c->profile ? c->dIpcWait : nullptr);
  c->fold_seq = 0;                    // consumed
  HIPCHK(c, hipGetLastError());
  c->g_parts = final_sum ? 0 : wgs;
  c->trace_parts = final_sum ? 0 : wgs;
  return PMF_OK;
}
// the folded exchange's consumer is an instantiation of its own (FOLD): the one-rank kernel carries none of it
template <int NT, bool BNMF>
int launch_h_gram(pmf_ctx* c) {
  return (c->fold_seq && c->ipc.nranks > 1) ? launch_h_gram_as<NT, BNMF, true>(c) : launch_h_gram_as<NT, BNMF, false>(c);
}

// NMF / BNMF: H step and G = H H^T in one launch.  false: not for this algorithm.
bool nmf_h_gram(pmf_ctx* c, int* rc) {
  if (c->algo != PMF_ALGO_NMF && c->algo != PMF_ALGO_BNMF) return false;   // RNMF: generic k_nmf_h
  if (c->nb > 1) return false;                                              // num_bases > 128: generic k_nmf_h
  const bool b = c->algo == PMF_ALGO_BNMF;
  switch (c->NT) {
    case 1: *rc = b ? launch_h_gram<1, true>(c) : launch_h_gram<1, false>(c); return true;
    case 2: *rc = b ? launch_h_gram<2, true>(c) : launch_h_gram<2, false>(c); return true;
    case 4: *rc = b ? launch_h_gram<4, true>(c) : launch_h_gram<4, false>(c); return true;
    case 8: *rc = b ? launch_h_gram<8, true>(c) : launch_h_gram<8, false>(c); return true;
  }
  return false;
}

int snmf_h_step(pmf_ctx* c) {   // snmf.py:72-91
  if (c->nb > 1) {                // num_bases > 128: the generic column-block kernel
    hipLaunchKernelGGL(k_nmf_h, dim3((unsigned)(c->np / 16)), dim3(256), (size_t)c->KP * 16 * sizeof(float), c->stream, c->dH,
                       (int64_t)c->np, c->np, c->KP, c->dPS, 3, 0.f, c->k, (int)c->n);
    return PMF_OK;
  }
  // num_bases <= 128: H in float64 (pmf_inv.h: k_snmf_h_f64), P / S in float64 inside the Gram-space loop
  PMFCHK(ensure_hd(c));
  const int64_t ldp = (int64_t)c->np + c->KP;
  const dim3 grid((unsigned)(c->np / 16));
#define PMF_SNMF_H64(NT_)                                                                                                    \
  if (c->ps_f64) hipLaunchKernelGGL((k_snmf_h_f64<NT_, double>), grid, dim3(64 * NT_), 0, c->stream, c->dHd, c->dH, c->np,   \
                                    (const double*)c->dPd, (int64_t)c->np, (const double*)c->dSd, (int64_t)c->KP, c->stop_arg); \
  else hipLaunchKernelGGL((k_snmf_h_f64<NT_, float>), grid, dim3(64 * NT_), 0, c->stream, c->dHd, c->dH, c->np,              \
                          (const float*)c->dPS, ldp, (const float*)c->dPS + c->np, ldp, c->stop_arg)
  switch (c->NT) {
    case 1: PMF_SNMF_H64(1); break;
    case 2: PMF_SNMF_H64(2); break;
    case 4: PMF_SNMF_H64(4); break;
    case 8: PMF_SNMF_H64(8); break;
    default: return fail(c, PMF_EINVAL, "bad NT");
  }
#undef PMF_SNMF_H64
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// dPS holds (W^T V | W^T W) of the current W summed over ALL ranks (ps_valid).  It does not depend
// on H, so repeated H steps with an unchanged W -- factorize(compute_w=False), the reference's
// documented "coefficients for an existing basis" use (nmf.py:56-65) -- reuse it: after the first
// iteration such a loop costs one k x n sized kernel per iteration and no pass over V at all.
int h_step_from_ps(pmf_ctx* c) {
  int hrc = PMF_OK;
  if (nmf_h_gram(c, &hrc)) {
    PMFCHK(hrc);
    c->g_valid = true;     // G (pad rows/cols are zero because the padded H rows are zero)
    c->num_valid = false;  // H changed
    c->ps_valid = true;
    c->trace_ready = c->want_trace;
    if (c->algo == PMF_ALGO_BNMF) { c->lamb_w *= 1.1; c->lamb_h *= 1.1; }   // bnmf.py:84-85
    return PMF_OK;
  }
  const size_t smem = (size_t)c->KP * 16 * sizeof(float);
  if (c->algo == PMF_ALGO_SNMF)
    PMFCHK(snmf_h_step(c));
  else
    hipLaunchKernelGGL(k_nmf_h, dim3((unsigned)(c->np / 16)), dim3(256), smem, c->stream, c->dH,
                       (int64_t)c->np, c->np, c->KP, c->dPS,
                       c->algo == PMF_ALGO_BNMF ? 1 : c->algo == PMF_ALGO_RNMF ? 2 : 0, (float)c->lamb_h,
                       c->k, (int)c->n);
  HIPCHK(c, hipGetLastError());
  c->g_valid = false; c->g_parts = 0; c->num_valid = false;
  c->ps_valid = true;    // dPS belongs to the current W (update_h never touches W)
  c->trace_ready = false;
  if (c->algo == PMF_ALGO_BNMF) { c->lamb_w *= 1.1; c->lamb_h *= 1.1; }   // bnmf.py:84-85
  return PMF_OK;
}

int ps_tiled(pmf_ctx* c) {   // dPS = (W^T V | W^T W) over this rank's rows
  if (c->nb > 1) return bigk_ps(c);
  if (use_csr(c)) return csr_ps(c);
  PMFCHK(colgemm(c));
  return reduce_slabs(c, c->nchunks);
}

int ensure_ps(pmf_ctx* c) {  // two-pass path: (re)build the all-rank (P | S) unless it is current
  if (c->ps_valid) return PMF_OK;
  PMFCHK(materialize_w(c));
  PMFCHK(ps_tiled(c));
  PMFCHK(allreduce_ps(c));
  c->ps_valid = true;
  return PMF_OK;
}

int nmf_update_h(pmf_ctx* c) {
  if (c->algo == PMF_ALGO_RNMF) {                // rnmf.py:100-107: H step on D = S - data, then update_s
    if (!c->s_valid) return fail(c, PMF_EINVAL, "RNMF: S does not exist yet (init_h / update_s create it, rnmf.py:94-98)");
    c->ps_valid = false;                         // D changed in the last update_s
    PMFCHK(ensure_ps(c));
    PMFCHK(h_step_from_ps(c));
    c->ps_valid = false;                         // (P | S) were built from D, not from V
    return rnmf_update_s(c);
  }
  PMFCHK(ensure_ps(c));
  return h_step_from_ps(c);
}

// One pass over V doing update_w AND the partials for update_h (pmf_fused.h): W is updated and the
// all-rank (P | S) of the NEW W is left in dPS.
int nmf_fused_pass(pmf_ctx* c) {
  c->ps_valid = false;
  c->trace_ready = false;       // <P,H>, <S,G> belong to the old W
  const float* Gsrc = c->dG;
  int ngp = 0;
  if (c->g_valid && c->g_parts > 0 && !c->fused8) { Gsrc = c->dGpart; ngp = c->g_parts; }   // partial sums, added by the kernel
  else PMFCHK(ensure_gram(c, 0.0));
  const bool rn = c->algo == PMF_ALGO_RNMF;     // rnmf.py:100-115: both contractions run on D = S - data
  if (rn && !c->s_valid) return fail(c, PMF_EINVAL, "RNMF: S does not exist yet (init_h / update_s create it, rnmf.py:94-98)");
  if (c->fused8) {               // the cooperative form (pmf_coop.h)
    stat_begin(c, SITE_FUSED);
    const int lrc8 = pmf_launch_coop(c->stream, rn ? FUSED_RNMF : c->algo == PMF_ALGO_BNMF ? FUSED_BNMF : FUSED_NMF, c->NT, c->np,
                                 rn ? c->dD : c->dV, c->dW, c->dH, c->dG, c->mp, c->fused_wgs, (float)c->lamb_w, c->dSlab,
                                 c->stop_arg);
    stat_end(c, SITE_FUSED);
    if (lrc8 != PMF_OK) return fail(c, lrc8, "cooperative one-pass kernel launch failed");
    HIPCHK(c, hipGetLastError());
    const int NTP8 = c->np / 16, KT8 = c->KP / 16;
    pmf_launch_reduce_slabs_coop(c->stream, c->dSlab, c->fused_wgs, c->coop_bt, NTP8, KT8, c->np, c->dPS, c->stop_arg);
    HIPCHK(c, hipGetLastError());
    PMFCHK(allreduce_ps(c));
    c->ps_valid = true;
    return PMF_OK;
  }
  const FusedCtl ctl = take_fused_ctl(c);
  hipEvent_t se0 = nullptr, se1 = nullptr;
  stat_pair(c, SITE_FUSED, &se0, &se1);          // (profiling: the pair rides on the dispatch itself, no barrier packets in the loop)
  const int lrc = pmf_launch_fused(c->stream, rn ? FUSED_RNMF : c->algo == PMF_ALGO_BNMF ? FUSED_BNMF : FUSED_NMF, c->NT,
                               c->np, rn ? c->dD : c->dV, c->dW, c->dH, Gsrc, c->mp, c->fused_wgs, (float)c->lamb_w,
                               c->dSlab, ctl, ngp, se0, se1);
  if (lrc != PMF_OK) return fail(c, lrc, "fused kernel launch failed");
  HIPCHK(c, hipGetLastError());
  {
    const int NTP = c->np / 16;
    const int ntu = c->NT * NTP + c->NT * (c->NT + 1) / 2;
    // the folded exchange: this launch pushes the rank's partial tiles to every peer, the H-step launch behind it waits for
    // the peers' and adds them in rank order (h_step_from_ps -> launch_h_gram) -- only inside nmf_fused_iteration, where that
    // launch is certain to follow on every rank
    const bool fold = c->fold_loop && c->opt_fold && c->ipc.nranks > 1 && ntu <= PMF_IPC_MAX_WGS && c->np / 64 <= PMF_HGRAM_MAX_WGS &&
                      (size_t)ps_elems(c) * sizeof(float) <= PMF_IPC_MAX_BYTES &&
                      (c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_BNMF) && c->nb == 1;
    const unsigned seq = fold ? ++c->ipc_seq : 0u;
    hipLaunchKernelGGL(k_reduce_slabs_tiles, dim3((unsigned)ntu), dim3(1024), 0, c->stream, c->dSlab,
                       c->fused_wgs, c->NT, NTP, c->np, c->dPS, c->stop_arg, fold ? c->ipc : IpcPeers{}, seq);
    HIPCHK(c, hipGetLastError());
    if (fold) {
      c->fold_seq = seq; c->fold_flags = ntu;
      ++c->ipc_calls; ++c->fold_calls;
      return PMF_OK;                  // dPS becomes the all-rank sum in the prologue of the H-step launch (ps_valid is set there)
    }
  }
  PMFCHK(allreduce_ps(c));
  c->ps_valid = true;
  return PMF_OK;
}

int nmf_fused_iteration(pmf_ctx* c) {
  c->fold_loop = true;
  const int prc = nmf_fused_pass(c);
  c->fold_loop = false;
  PMFCHK(prc);
  PMFCHK(h_step_from_ps(c));
  if (c->algo == PMF_ALGO_RNMF) {               // rnmf.py:107: update_h ends with update_s
    c->ps_valid = false;                        // (P | S) were built from D, not from V
    return rnmf_update_s(c);
  }
  return PMF_OK;
}

}  // namespace
