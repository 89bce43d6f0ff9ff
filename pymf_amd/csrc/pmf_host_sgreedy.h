// pmf_host_sgreedy.h -- SIVM_SGREEDY: the round driver of the exact greedy max-volume selection of a SIVM context (kernels: pmf_sgreedy.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// the distance table [64][np] float32, inv(CM_S) [64][64], scale_t and the rounds' volumes: buffers of the context, on first use
int sgreedy_alloc(pmf_ctx* c) {
  if (c->dSgTab) return PMF_OK;
  PMFCHK(dalloc(c, &c->dSgTab, (size_t)PMF_SGREEDY_MAX_T * c->np));
  PMFCHK(dalloc(c, &c->dSgM, (size_t)PMF_SGREEDY_MAX_T * PMF_SGREEDY_MAX_T));
  PMFCHK(dalloc(c, &c->dSgVol, (size_t)PMF_SGREEDY_MAX_T + 4));   // [0 .. 63] the volumes (the close writes one slot past the last), [66] scale_t
  return PMF_OK;
}

// dynamic LDS of k_sgreedy_pass in round t: x, then M in blocks of PMF_SGREEDY_BLK
size_t sgreedy_pass_smem(int R, int t) {
  const int tp = (t + 1 + PMF_SGREEDY_BLK - 1) / PMF_SGREEDY_BLK * PMF_SGREEDY_BLK;
  return (size_t)((R + 3) & ~3) * sizeof(float) + (size_t)tp * tp * sizeof(double);
}

// SIVM_SGREEDY.update_w (sivm_sgreedy.py:96-133) on A [R rows][ld], candidates its C columns: init_sivm's plain rounds in the
// context's metric (three launches of k_laesa_pass for 'fastmap', one for 'origin'), then nsel - 1 rounds of k_sgreedy_step and
// k_sgreedy_pass, then the closing reduce, which also leaves the last round's volume.  Nothing is read by the host in between.
int sgreedy_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int metric, bool origin, const SivmBufs& b) {
  PMFCHK(sgreedy_alloc(c));
  ColselArgs l{};
  PanelChain ch = colsel_begin(l, A, ld, R, C, b);
  l.fixed_idx = origin ? -1 : 0;
  l.sel_pos = -1; l.plain = 1;
  for (int q = 0; q < (origin ? 1 : 3); ++q) {
    l.use_fixed = chain_next(ch, l) == 0;
    laesa_launch_pass(c, l, ch.wgs, metric);
    HIPCHK(c, hipGetLastError());
  }
  c->sg_have_vol = true;
  if (nsel == 1) return chain_close(c, ch, C, 0, true, origin, b.scal);

  const size_t smem_max = sgreedy_pass_smem(PMF_SIVM_MAX_M, PMF_SGREEDY_MAX_T - 1);
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};      // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sgreedy_pass), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max));
    attr_done = true;
  }
  SgreedyArgs a{};
  static_cast<ColsweepArgs&>(a) = l;               // the same matrix and partition
  a.d2 = c->dSgTab; a.M = c->dSgM; a.sc = c->dSgVol + PMF_SGREEDY_MAX_T + 2; a.vol = c->dSgVol;
  a.select = b.select;
  a.origin = origin ? 1 : 0;
  for (int t = 1; t < nsel; ++t) {
    chain_next(ch, a);                             // (the step reads the partials its pass reads)
    a.t = t;
    hipLaunchKernelGGL(k_sgreedy_step, dim3(1), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    stat_begin(c, SITE_SGREEDY);
    hipLaunchKernelGGL(k_sgreedy_pass, dim3((unsigned)ch.wgs), dim3(256), sgreedy_pass_smem(R, t), c->stream, a);
    stat_end(c, SITE_SGREEDY);
    HIPCHK(c, hipGetLastError());
  }
  // the last argmax into select[nsel - 1]; its score -- the last round's volume -- into vol[nsel - 2] (k_sivm_close's maxd slot;
  // the logarithm it stores next to it lands in the unused slot behind)
  PMFCHK(chain_close(c, ch, C, nsel - 1, true, false, c->dSgVol + (nsel - 2)));
  // the reference's order of select, so that W = V[:, select] and the rows of H are in it too
  hipLaunchKernelGGL(k_sgreedy_order, dim3(1), dim3(64), 0, c->stream, b.select, nsel);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// pmf_sivm_get_volumes: the num_bases - 1 volumes of the last SIVM_SGREEDY selection
int sgreedy_get_volumes(pmf_ctx* c, double* vol) {
  if (c->k > 1) HIPCHK(c, hipMemcpyAsync(vol, c->dSgVol, (size_t)(c->k - 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

}  // namespace
