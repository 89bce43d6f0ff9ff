// pmf_host_snmf.h -- SNMF: CSR data and the pipelined W write, the inverse, the one-pass and the Gram-space iteration (kernels: pmf_csr.h, pmf_inv.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// ---- CSR (SNMF) ----------------------------------------------------------------------------
template <int NT>
int launch_csr_w_blocks(pmf_ctx* c, hipStream_t stream, const float* Mbuf, int reserve) {
  const size_t mbytes = (size_t)c->np * c->KP * sizeof(float);
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_csr_w_blocks<NT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    attr_done = true;
  }
  int dev = 0, cus = 256;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
  const int64_t nblk = c->mp / 16;
  const int64_t nwg_full = (nblk + 15) / 16;          // one workgroup (16 waves) per 16 blocks = 256 rows = one contiguous piece of W
  // Round 4 (tools/csrw_lab.hip): a NON-persistent grid -- every workgroup writes ONE contiguous 256-row piece of W and
  // leaves, the pieces swept through memory in dispatch order -- with M read from L2 (64 KiB, resident; no LDS image to
  // stage per workgroup) stores at 6.75 TB/s where 512 persistent workgroups striding through W reach 5.4 (a pure store
  // stream of that strided shape: 5.1-5.6; hipMemsetAsync: 6.45).  Taken when the grid is several waves of workgroups deep.
  if (nwg_full >= (int64_t)8 * cus && mbytes <= (size_t)1 << 20) {
    hipLaunchKernelGGL((k_csr_w_blocks<NT>), dim3((unsigned)nwg_full), dim3(1024), 0, stream, c->dIndptr, c->dIndices, c->dVals,
                       nblk, c->np, Mbuf, c->dW, 0);
    HIPCHK(c, hipGetLastError());
    return PMF_OK;
  }
  const int in_lds = mbytes <= 128 * 1024;
  const size_t smem = in_lds ? mbytes : 0;
  const int per_cu = smem <= 80 * 1024 ? 2 : 1;     // workgroups of 16 waves per CU
  const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nwg_full, (int64_t)cus * per_cu - reserve));
  hipLaunchKernelGGL((k_csr_w_blocks<NT>), dim3(wgs), dim3(1024), smem, stream, c->dIndptr, c->dIndices, c->dVals,
                     nblk, c->np, Mbuf, c->dW, in_lds);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// W = V M, M = H^T inv(H H^T) (np x KP) in dW1 (snmf_inverse formed it) -- or, for the pipelined write, in Mbuf on `stream`
int csr_w(pmf_ctx* c, hipStream_t stream = nullptr, const float* Mbuf = nullptr, int reserve = 0) {
  if (!stream) stream = c->stream;
  if (!Mbuf) Mbuf = c->dW1;
  switch (c->NT) {
    case 1: return launch_csr_w_blocks<1>(c, stream, Mbuf, reserve);
    case 2: return launch_csr_w_blocks<2>(c, stream, Mbuf, reserve);
    case 4: return launch_csr_w_blocks<4>(c, stream, Mbuf, reserve);
    case 8: return launch_csr_w_blocks<8>(c, stream, Mbuf, reserve);
  }
  return fail(c, PMF_EINVAL, "bad NT");
}

// The pipelined W write of the snmf_gram = 2 loop on CSR data.
bool w_pipe_on(const pmf_ctx* c) { return c->opt_snmf_gram == 2 && use_csr(c) && c->opt_w_pipe > 0 && (size_t)2 * c->np * c->KP <= (size_t)std::max<int64_t>(c->mp, c->np) * c->KP; }
float* w_pipe_mbuf(pmf_ctx* c, int64_t it) { return c->dW1 + (size_t)(it & 1) * c->np * c->KP; }
int w_pipe_init(pmf_ctx* c) {
  if (c->w_stream) return PMF_OK;
  HIPCHK(c, hipStreamCreateWithFlags(&c->w_stream, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b) {
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_mt[b], hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_w[b], hipEventDisableTiming));
  }
  return PMF_OK;
}
// every write enqueued on the side stream has finished before anything later on the main stream runs
int w_pipe_join(pmf_ctx* c) {
  for (int b = 0; b < 2; ++b)
    if (c->ev_w_pending[b]) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_w[b], 0)); c->ev_w_pending[b] = false; }
  return PMF_OK;
}

int csr_ps(pmf_ctx* c) {   // slabs: S part by the dense W^T W kernel, P part by the CSR scatter
  const size_t smem = (size_t)c->np * c->KP * sizeof(float);
  if (smem > 160 * 1024) return fail(c, PMF_EINVAL, "CSR path: n * num_bases too large for the LDS accumulator");
  PMFCHK(colgemm(c, /*with_v=*/false));
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_csr_p<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_csr_p<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done = true;
  }
  if (c->KP <= 64)
    hipLaunchKernelGGL((k_csr_p<1>), dim3((unsigned)c->nchunks), dim3(256), smem, c->stream, c->dIndptr,
                       c->dIndices, c->dVals, c->mp, c->rows_per_chunk, c->KP, c->np, c->dW, c->dSlab);
  else
    hipLaunchKernelGGL((k_csr_p<2>), dim3((unsigned)c->nchunks), dim3(256), smem, c->stream, c->dIndptr,
                       c->dIndices, c->dVals, c->mp, c->rows_per_chunk, c->KP, c->np, c->dW, c->dSlab);
  HIPCHK(c, hipGetLastError());
  return reduce_slabs(c, c->nchunks);
}

// ---- SNMF -----------------------------------------------------------------------------------
// inv(H H^T) in float64 (Gauss-Jordan in registers, identity on the padding), then M^T = inv(H H^T) H in
// float64, rounded once: dMT [KP][np] for the dense kernels, dW1 = M [np][KP] for the CSR kernels.
// snmf.py:69: np.linalg.inv raises LinAlgError("Singular matrix") on a zero pivot; the inverse kernels raise
// dSing instead, read back wherever the host synchronises anyway (end of pmf_update_w / pmf_factorize / a streamed pass).
int check_singular(pmf_ctx* c) {
  if (c->algo != PMF_ALGO_SNMF || !c->dSing) return PMF_OK;
  int flag = 0;
  HIPCHK(c, hipMemcpyAsync(&flag, c->dSing, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!flag) return PMF_OK;
  HIPCHK(c, hipMemsetAsync(c->dSing, 0, sizeof(int), c->stream));
  return fail(c, PMF_ESINGULAR, "SNMF: H H^T is singular (the reference's np.linalg.inv raises LinAlgError, snmf.py:69)");
}

int launch_inverse(pmf_ctx* c) {   // dGinvD = inv(dGd), float64
  if (!c->dSing) PMFCHK(dalloc(c, &c->dSing, 1));
  if (c->KP <= 64) {                       // blocked Gauss-Jordan on the float64 MFMA (pmf_inv.h)
    hipLaunchKernelGGL((k_inverse_spd_mfma<4>), dim3(1), dim3(256), 0, c->stream, c->dGd, c->KP, c->k, c->dGinvD, c->stop_arg, c->dSing);
  } else if (c->KP <= 128) {
    hipLaunchKernelGGL((k_inverse_spd_mfma<8>), dim3(1), dim3(1024), 0, c->stream, c->dGd, c->KP, c->k, c->dGinvD, c->stop_arg, c->dSing);
  } else {                         // num_bases > 128: the matrix in L2, a cooperative grid (k_inverse_spd_big)
    const size_t E = (size_t)c->KP * c->KP;
    if (!c->dInvA) { PMFCHK(dalloc(c, &c->dInvA, E)); PMFCHK(dalloc(c, &c->dInvB, E)); }
    // dGd stays intact (g_valid covers it): the elimination runs on a copy; a stopped free-running loop keeps dGinvD
    HIPCHK(c, hipMemcpyAsync(c->dInvA, c->dGd, E * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    int dev = 0, cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cus, (int64_t)E / 4096));
    double *a_ = c->dInvA, *b_ = c->dInvB, *o_ = c->dGinvD;
    int kp_ = c->KP, k_ = c->k;
    const int* stop_ = c->stop_arg;
    int* sing_ = c->dSing;
    void* args[] = {&a_, &b_, &kp_, &k_, &o_, &stop_, &sing_};
    HIPCHK(c, hipLaunchCooperativeKernel(reinterpret_cast<const void*>(&k_inverse_spd_big), dim3(wgs), dim3(1024), args, 0,
                                         c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

int snmf_inverse(pmf_ctx* c) {
  PMFCHK(ensure_gram(c, 1.0));
  PMFCHK(launch_inverse(c));
  if (h_in_f64(c)) {
    PMFCHK(ensure_hd(c));
    hipLaunchKernelGGL(k_snmf_mt<double>, dim3((unsigned)(c->np / 16), (unsigned)(c->KP / 16)), dim3(64), 0, c->stream, c->dHd,
                       (int64_t)c->np, c->np, c->KP, c->dGinvD, use_csr(c) ? (float*)nullptr : c->dMT,
                       use_csr(c) ? c->dW1 : (float*)nullptr, (double*)nullptr, (const int*)nullptr);
  } else {
    hipLaunchKernelGGL(k_snmf_mt<float>, dim3((unsigned)(c->np / 16), (unsigned)(c->KP / 16)), dim3(64), 0, c->stream, c->dH,
                       (int64_t)c->np, c->np, c->KP, c->dGinvD, use_csr(c) ? (float*)nullptr : c->dMT,
                       use_csr(c) ? c->dW1 : (float*)nullptr, (double*)nullptr, (const int*)nullptr);
  }
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

int snmf_update_w(pmf_ctx* c) {
  if (c->fused_wgs > 0 && !use_csr(c)) return snmf_fused_pass(c);   // as nmf_update_w: one pass, (P | S) kept for update_h
  PMFCHK(snmf_inverse(c));
  if (use_csr(c)) return csr_w(c);
  return rowgemm<EPI_STORE>(c, c->dV, c->np, c->np, c->dMT, c->np, nullptr, nullptr, c->dW);   // W = V M^T
}

// SNMF: update_w and the partials of update_h in ONE pass over V (dense data, fused shapes).
int snmf_fused_pass(pmf_ctx* c) {
  c->ps_valid = false;
  c->trace_ready = false;
  PMFCHK(snmf_inverse(c));
  const FusedCtl ctl = take_fused_ctl(c);
  stat_begin(c, SITE_FUSED);
  const int lrc = pmf_launch_fused(c->stream, FUSED_SNMF, c->NT, c->np, c->dV, c->dW, c->dMT, nullptr, c->mp,
                                   c->fused_wgs, 0.f, c->dSlab, ctl, 0);
  stat_end(c, SITE_FUSED);
  if (lrc != PMF_OK) return fail(c, lrc, "fused SNMF kernel launch failed");
  HIPCHK(c, hipGetLastError());
  {
    const int NTP = c->np / 16;
    const int ntu = c->NT * NTP + c->NT * (c->NT + 1) / 2;
    hipLaunchKernelGGL(k_reduce_slabs_tiles, dim3((unsigned)ntu), dim3(1024), 0, c->stream, c->dSlab,
                       c->fused_wgs, c->NT, NTP, c->np, c->dPS, c->stop_arg, IpcPeers{}, 0u);
    HIPCHK(c, hipGetLastError());
  }
  PMFCHK(allreduce_ps(c));
  c->ps_valid = true;
  return PMF_OK;
}

int snmf_fused_iteration(pmf_ctx* c) {
  PMFCHK(snmf_fused_pass(c));
  return h_step_from_ps(c);
}

// out [np][np] float64 = the Gram matrix of the columns of a CSR image (indptr [>= lines + 1], indices < np, vals; nnz entries in
// `lines` lines): k_csr_gram's per-workgroup images in exact fixed point (pmf_csr.h), added up as integers.  np is a multiple of
// 64; the slabs and the word of the largest |v| stay with the context (one image width per context).
int csr_gram_f64(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz, int64_t lines, int np,
                 double* out) {
  const size_t E = (size_t)np * np;
  const size_t T2 = 2 * gram_tri(np);                                // two 64-bit limbs per entry of the upper triangle
  const int use_lds = T2 * sizeof(unsigned long long) + gram_stage_bytes() <= 160 * 1024;
  const int wgs = use_lds ? 256 : 32;            // global images are T2 words each: fewer of them
  // the grids of the two limbs from the largest |v|: |v| < 2^e  ->  u1 = 2^(2e-32), u2 = 2^(2e-64)
  if (!c->dVmaxBits) PMFCHK(dalloc(c, &c->dVmaxBits, (size_t)1));
  unsigned* mxbits = c->dVmaxBits;
  HIPCHK(c, hipMemsetAsync(mxbits, 0, sizeof(unsigned), c->stream));
  if (nnz > 0) {
    hipLaunchKernelGGL(k_absmax_bits_f32, dim3((unsigned)std::min<int64_t>((nnz + 255) / 256, 2048)), dim3(256), 0, c->stream, vals, nnz, mxbits);
    HIPCHK(c, hipGetLastError());
  }
  unsigned hb = 0;
  HIPCHK(c, hipMemcpyAsync(&hb, mxbits, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float vmax;
  std::memcpy(&vmax, &hb, sizeof(float));
  const int finite = std::isfinite(vmax) ? 1 : 0;
  int ex = 0;
  if (finite && vmax > 0.f) (void)std::frexp(vmax, &ex);             // vmax = f 2^ex, f in [0.5, 1): |v| < 2^ex
  GramScale gs;
  gs.u1 = std::ldexp(1.0, 2 * ex - 32); gs.inv_u1 = std::ldexp(1.0, 32 - 2 * ex); gs.inv_u2 = std::ldexp(1.0, 64 - 2 * ex);
  // per-workgroup images of C: kept with the context (34 MiB at n = 128); zeroed only where the kernel adds
  // into them directly (LDS images are written out whole)
  if (!c->dCslabs) PMFCHK(dalloc_raw(c, &c->dCslabs, (size_t)wgs * T2));   // (64-bit limbs)
  unsigned long long* slabs = reinterpret_cast<unsigned long long*>(c->dCslabs);
  if (!use_lds) HIPCHK(c, hipMemsetAsync(slabs, 0, (size_t)wgs * T2 * sizeof(unsigned long long), c->stream));
  const size_t smem = (use_lds ? T2 * sizeof(unsigned long long) : 0) + gram_stage_bytes();
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_csr_gram), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(160 * 1024)));
    attr_done = true;
  }
  hipLaunchKernelGGL(k_csr_gram, dim3((unsigned)wgs), dim3(64 * GRAM_WAVES), smem, c->stream, indptr, indices, vals, lines, np, slabs,
                     use_lds, gs);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_csr_gram_sum, dim3((unsigned)((E + 63) / 64)), dim3(256), 0, c->stream, slabs, wgs, np, out, gs, finite);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// ---- SNMF in Gram space ---------------------------------------------------------------------------
// snmf.py:67-70 makes W a LINEAR function of the data once H is given: W = V M, M = H^T inv(H H^T).
// Everything update_h (snmf.py:72-91) takes from W are XW = V^T W and WW = W^T W, i.e.
//     P = W^T V = M^T (V^T V) = M^T C,      S = W^T W = M^T C M = P M,      C = V^T V  (n x n),
// and C does not change during factorize().  So a loop that runs update_w AND update_h needs ONE pass
// over V (C, float64, all-reduced once across the ranks) and then iterates on k x n sized data only:
// G = H H^T -> inv -> M^T (all float64) -> P = M^T C -> S = P M -> the H step -> the error through the
// trace identity (same P, S).  W is materialised once, after the last iteration (W = V M with the M of
// that iteration: exactly the W the reference holds then).  No per-iteration pass over V or W, no
// per-iteration collective; results agree with the pass-per-iteration form to rounding (P, S now come
// out of float64 arithmetic).  CSR data: C by k_csr_gram (pmf_csr.h), dense data: gram_vtv.
int ensure_vgram(pmf_ctx* c) {
  if (c->c_valid) return PMF_OK;
  const int np = c->np;
  if (!c->dC) PMFCHK(dalloc(c, &c->dC, (size_t)np * np));
  if (!c->dMTd) PMFCHK(dalloc(c, &c->dMTd, (size_t)c->KP * np));
  if (!c->dPd) PMFCHK(dalloc(c, &c->dPd, (size_t)c->KP * np));
  if (use_csr(c)) {
    const size_t E = (size_t)np * np;
    PMFCHK(csr_gram_f64(c, c->dIndptr, c->dIndices, c->dVals, c->nnz, c->m, np, c->dC));
    PMFCHK(allreduce_sum(c, c->dC, E, true));
  } else {
    DevTemps tmp;
    const int64_t blocks16 = c->mp / 16;
    int gchunks = (int)std::min<int64_t>(512, blocks16);
    const int rpc = (int)((blocks16 + gchunks - 1) / gchunks) * 16;   // (small chunks on purpose: fp32 sums inside a chunk, float64 across)
    gchunks = (int)((c->mp + rpc - 1) / rpc);
    float* slab = nullptr;
    PMFCHK(talloc(c, tmp, &slab, (size_t)gchunks * 128 * (np + 128)));
    PMFCHK(gram_vtv(c, c->dC, slab, gchunks, rpc));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the scratch is freed on return
  }
  c->c_valid = true;
  return PMF_OK;
}

constexpr int PMF_GRAM_MAX_NP = 1024;   // C is np x np float64 (8 MiB at the limit)

// Worth it?  CSR data: always (C costs a few ms on the host).  Dense data: forming C is 2 m n^2 flop, a
// pass-per-iteration step 4 m n k: from about n / 2k iterations on (or when C is already there).
bool snmf_gram_ok(const pmf_ctx* c, int niter) {
  if (c->algo != PMF_ALGO_SNMF || c->np > PMF_GRAM_MAX_NP) return false;
  if (c->opt_snmf_gram == 0) return false;
  if (use_csr(c)) return true;
  return c->opt_snmf_gram >= 1 || c->c_valid || (int64_t)2 * c->k * niter >= c->n;
}

int snmf_gram_iteration(pmf_ctx* c) {
  const int np = c->np, KP = c->KP;
  const int64_t ldp = (int64_t)np + KP;
  c->ps_valid = false;
  c->trace_ready = false;
  PMFCHK(ensure_gram(c, 1.0));
  PMFCHK(launch_inverse(c));
  const bool pipe = w_pipe_on(c);
  float* mcsr = c->dW1;
  if (pipe) {                  // M of this iteration goes into the buffer the write before last has finished reading
    PMFCHK(w_pipe_init(c));
    const int b = (int)(c->w_pipe_it & 1);
    if (c->ev_w_pending[b]) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_w[b], 0)); c->ev_w_pending[b] = false; }
    mcsr = w_pipe_mbuf(c, c->w_pipe_it);
  }
  const bool h64 = h_in_f64(c);
  if (h64) {
    PMFCHK(ensure_hd(c));
    hipLaunchKernelGGL(k_snmf_mt<double>, dim3((unsigned)(np / 16), (unsigned)(KP / 16)), dim3(64), 0, c->stream, c->dHd, (int64_t)np, np, KP,
                       c->dGinvD, use_csr(c) ? (float*)nullptr : c->dMT, use_csr(c) ? mcsr : (float*)nullptr, c->dMTd, c->stop_arg);
  } else {
    hipLaunchKernelGGL(k_snmf_mt<float>, dim3((unsigned)(np / 16), (unsigned)(KP / 16)), dim3(64), 0, c->stream, c->dH, (int64_t)np, np, KP,
                       c->dGinvD, use_csr(c) ? (float*)nullptr : c->dMT, use_csr(c) ? mcsr : (float*)nullptr, c->dMTd, c->stop_arg);
  }
  HIPCHK(c, hipGetLastError());
  if (pipe) {                  // W = V M on the side stream, beside everything that follows here (nothing below reads W)
    const int b = (int)(c->w_pipe_it & 1);
    HIPCHK(c, hipEventRecord(c->ev_mt[b], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->w_stream, c->ev_mt[b], 0));
    // the launch's own HIP events, on the stream it runs on -- sampled like every timed site (profile_every): the pair sits
    // BETWEEN two writes of a loop that is bound by exactly these writes
    const bool timed_w = c->profile && c->stat.site == SITE_MATERIALIZE && (c->stat.seen++ % c->stat.every == 0);
    if (timed_w) {
      KernelStat& st = c->stat;
      if (st.used + 2 > st.ev.size()) for (int q = 0; q < 2; ++q) { hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) st.ev.push_back(e); }
      if (st.used + 2 <= st.ev.size()) (void)hipEventRecord(st.ev[st.used], c->w_stream);
    }
    PMFCHK(csr_w(c, c->w_stream, mcsr, c->opt_w_pipe));
    if (timed_w && c->stat.used + 2 <= c->stat.ev.size()) {
      (void)hipEventRecord(c->stat.ev[c->stat.used + 1], c->w_stream);
      c->stat.used += 2;
    }
    HIPCHK(c, hipEventRecord(c->ev_w[b], c->w_stream));
    c->ev_w_pending[b] = true;
    ++c->w_pipe_it;
  }
  // P = M^T C  (KP x np), float64 kept for S, float32 into (P | S)
  hipLaunchKernelGGL((k_dgemm_mfma<false>), dim3((unsigned)(np / 16), (unsigned)(KP / 16)), dim3(64), 0, c->stream, c->dMTd,
                     (int64_t)np, c->dC, (int64_t)np, np, c->dPd, (int64_t)np, c->dPS, ldp, c->stop_arg);
  HIPCHK(c, hipGetLastError());
  // S = P M = P (M^T)^T  (KP x KP)
  hipLaunchKernelGGL((k_dgemm_mfma<true>), dim3((unsigned)(KP / 16), (unsigned)(KP / 16)), dim3(64), 0, c->stream, c->dPd,
                     (int64_t)np, c->dMTd, (int64_t)np, np, h64 ? c->dSd : (double*)nullptr, (int64_t)KP, c->dPS + np, ldp, c->stop_arg);
  HIPCHK(c, hipGetLastError());
  c->w_implicit = !pipe;      // dW is stale from here on: W = V M with the M just formed (pipelined: being written already)
  c->ps_valid = true;         // (P | S) of that W, all ranks (C is all-reduced)
  if (c->opt_snmf_gram == 2 && !pipe) PMFCHK(materialize_w(c));   // W rewritten in every iteration, as the reference's update_w does
  c->ps_valid = true;
  c->ps_f64 = h64;            // the H step takes P and S in float64 (dPd, dSd), not their float32 roundings in (P | S)
  const int hrc = h_step_from_ps(c);
  c->ps_f64 = false;
  c->psd_fresh = h64 && hrc == PMF_OK;     // the error of this iteration takes <P,H>, <S H,H> from the float64 P, S and H
  return hrc;
}

// W = V M for the M the last Gram-space iteration formed (dMT dense / dW1 CSR).
int materialize_w(pmf_ctx* c) {
  PMFCHK(w_pipe_join(c));     // (a pipelined write still in flight on the side stream)
  if (!c->w_implicit) return PMF_OK;
  c->w_implicit = false;
  stat_begin(c, SITE_MATERIALIZE);
  int rc = PMF_OK;
  if (use_csr(c)) {
    const bool keep_ps = c->ps_valid;
    rc = csr_w(c);
    c->ps_valid = keep_ps;
  } else {
    if (c->algo == PMF_ALGO_CNMF) {   // W = V G: the "M^T" operand is the float32 rounding of G^T
      const int64_t E = (int64_t)c->KP * c->np;
      hipLaunchKernelGGL(k_f64_to_f32, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, c->stream, c->dGT, E, c->dMT);
      HIPCHK(c, hipGetLastError());
    }
    rc = rowgemm<EPI_STORE>(c, c->dV, c->np, c->np, c->dMT, c->np, nullptr, nullptr, c->dW);
  }
  stat_end(c, SITE_MATERIALIZE);
  return rc;
}

// pmf_kernel_stats names the instantiation that runs: the launch itself writes it (choose_stat_site cannot know the dispatch)
void name_csr_pass(pmf_ctx* c, const char* kernel) {
  if (c->stat.site == SITE_CSR_PASS && c->stat.name != kernel) c->stat.name = kernel;
}

// CSR SNMF: update_w and the (P | S) partials of update_h in one pass over the CSR rows.
template <int NT>
int launch_csr_fused(pmf_ctx* c, int wgs) {
  static const std::string kname = "k_snmf_csr_fused<" + std::to_string(NT) + ">";
  name_csr_pass(c, kname.c_str());
  const size_t smem = ((size_t)2 * c->np * c->KP + 4 * 16 * c->KP) * sizeof(float);
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_snmf_csr_fused<NT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done = true;
  }
  const int nblk = (int)(c->mp / 16), nw = wgs * 4;
  hipLaunchKernelGGL((k_snmf_csr_fused<NT>), dim3(wgs), dim3(256), smem, c->stream, c->dIndptr, c->dIndices,
                     c->dVals, nblk / nw, nblk % nw, c->np, c->dW1, c->dW, c->dSlab);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

template <int NT, int NTP>
int launch_csr_mfma(pmf_ctx* c, int wgs) {
  static const std::string kname = "k_snmf_csr_mfma<" + std::to_string(NT) + "," + std::to_string(NTP) + ">";
  name_csr_pass(c, kname.c_str());
  const size_t smem = ((size_t)16 * NTP * 16 * NT + 64 * 16 * NTP) * sizeof(float) + 16;
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_snmf_csr_mfma<NT, NTP>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    attr_done = true;
  }
  const int nblk = (int)(c->mp / 16), nw = wgs * 4;
  hipLaunchKernelGGL((k_snmf_csr_mfma<NT, NTP>), dim3(wgs), dim3(256), smem, c->stream, c->dIndptr,
                     c->dIndices, c->dVals, nblk / nw, nblk % nw, c->dW1, c->dW, c->dSlab);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// MFMA variant for the register-resident P shapes; false: not covered (LDS-atomic kernel instead)
bool csr_mfma(pmf_ctx* c, int wgs, int* rc) {
  if (c->np % 16) return false;
  const int key = c->NT * 100 + c->np / 16;
  switch (key) {
    case 808: *rc = launch_csr_mfma<8, 8>(c, wgs); return true;
    case 408: *rc = launch_csr_mfma<4, 8>(c, wgs); return true;
    case 404: *rc = launch_csr_mfma<4, 4>(c, wgs); return true;
    case 208: *rc = launch_csr_mfma<2, 8>(c, wgs); return true;
    case 108: *rc = launch_csr_mfma<1, 8>(c, wgs); return true;
    case 104: *rc = launch_csr_mfma<1, 4>(c, wgs); return true;
  }
  return false;
}

bool csr_fused_ok(const pmf_ctx* c) {
  const size_t smem = ((size_t)2 * c->np * c->KP + 4 * 16 * c->KP) * sizeof(float);
  return use_csr(c) && smem <= 160 * 1024;
}

int snmf_csr_fused_iteration(pmf_ctx* c) {
  c->ps_valid = false;
  PMFCHK(snmf_inverse(c));            // leaves M = H^T inv(H H^T) in dW1
  int dev = 0, cus = 256;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
  int wgs = (int)std::min<int64_t>((c->mp / 16 + 3) / 4, cus);
  wgs = std::min(wgs, c->nchunks > 0 ? std::max(c->nchunks, 1) : wgs);   // slab capacity
  stat_begin(c, SITE_CSR_PASS);
  int mrc = PMF_OK;
  if (csr_mfma(c, wgs, &mrc)) {
    stat_end(c, SITE_CSR_PASS);
    PMFCHK(mrc);
    PMFCHK(reduce_slabs(c, wgs));
    PMFCHK(allreduce_ps(c));
    c->ps_valid = true;
    return h_step_from_ps(c);
  }
  switch (c->NT) {
    case 1: PMFCHK(launch_csr_fused<1>(c, wgs)); break;
    case 2: PMFCHK(launch_csr_fused<2>(c, wgs)); break;
    case 4: PMFCHK(launch_csr_fused<4>(c, wgs)); break;
    // NT = 8 arrives here with np = 64 only (np = 128 is k_snmf_csr_mfma<8,8>, np >= 192 fails csr_fused_ok: 2 np KP floats
    // beyond 160 KiB): more than 64 bases on at most 64 columns, so H H^T has rank <= n < num_bases and the step has no
    // meaning (snmf.py:69 inverts a singular matrix).  The instantiation stays so that such a call behaves as on every other
    // shape and does not end in "bad NT"; no solvable problem runs it (tests/snmf_csr_cases.py: dead_forms).
    case 8: PMFCHK(launch_csr_fused<8>(c, wgs)); break;
    default: return fail(c, PMF_EINVAL, "bad NT");
  }
  stat_end(c, SITE_CSR_PASS);
  PMFCHK(reduce_slabs(c, wgs));
  PMFCHK(allreduce_ps(c));
  c->ps_valid = true;
  return h_step_from_ps(c);
}

int snmf_update_h(pmf_ctx* c) {
  PMFCHK(ensure_ps(c));
  return h_step_from_ps(c);
}

}  // namespace
