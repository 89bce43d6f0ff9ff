// pmf_host_colsel.h -- LAESA and GMAP: the round drivers of the two lighter selection rules of a SIVM context (kernels: pmf_colsel.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// what every launch of either rule shares: the matrix, the buffers (SivmBufs: state holds >= 2 ld doubles) and the partition
ColselArgs colsel_args(const float* A, int64_t ld, int R, int C, const SivmBufs& b, int ppw) {
  ColselArgs a{};
  a.V = A;
  a.st0 = b.state; a.st1 = b.state + ld;
  a.select = b.select; a.scal = b.scal;
  a.np = ld; a.m = R; a.n = C;
  a.npanels = (int)(ld / 64); a.panels_per_wg = ppw;
  return a;
}

// launch p of a chain reads the partials that launch p - 1 wrote
void colsel_flip(ColselArgs& a, const SivmBufs& b, size_t p, int wgs) {
  const int out = (int)(p & 1), in = out ^ 1;
  a.pscore_in = b.part + in * PMF_CL_MAX_WGS; a.pidx_in = b.pidx + in * PMF_CL_MAX_WGS;
  a.pscore_out = b.part + out * PMF_CL_MAX_WGS; a.pidx_out = b.pidx + out * PMF_CL_MAX_WGS;
  a.nprev = p == 0 ? 0 : wgs;
}

int colsel_close(pmf_ctx* c, const SivmBufs& b, size_t launches, int wgs, int C, int nsel, int take_maxd, int origin_first) {
  const int last = (int)((launches - 1) & 1);
  hipLaunchKernelGGL(k_sivm_close, dim3(1), dim3(256), 0, c->stream, (const double*)(b.part + last * PMF_CL_MAX_WGS),
                     (const int*)(b.pidx + last * PMF_CL_MAX_WGS), wgs, C, nsel - 1, take_maxd, origin_first, b.select, b.scal);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// LAESA.update_w (laesa.py:63-82) on A [R rows][ld], candidates its C columns: the rounds of sivm_rounds -- nsel + 2 ('fastmap')
// or nsel ('origin') launches of k_laesa_pass back to back -- and the closing reduce.  The state needs no clearing: the first
// recurrence round writes it whole.
int laesa_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int metric, bool origin, const SivmBufs& b) {
  int ppw = 0, wgs = 0;
  panel_partition((int)(ld / 64), PMF_CL_MAX_WGS, &ppw, &wgs);
  ColselArgs a = colsel_args(A, ld, R, C, b, ppw);
  a.fixed_idx = origin ? -1 : 0;
  const std::vector<SivmRound> rounds = sivm_rounds(nsel, origin);
  const dim3 grid((unsigned)wgs), block(256);
  const size_t smem = (size_t)R * sizeof(float);
  for (size_t p = 0; p < rounds.size(); ++p) {
    const SivmRound& r = rounds[p];
    colsel_flip(a, b, p, wgs);
    a.use_fixed = p == 0 || (origin && r.l == 1);
    a.sel_pos = r.sel_pos; a.take_maxd = r.l == 1; a.plain = r.plain; a.first = r.l == 1;
    stat_begin(c, SITE_LAESA);
    switch (metric) {
      case PMF_SIVM_L2: hipLaunchKernelGGL(k_laesa_pass<PMF_SIVM_L2>, grid, block, smem, c->stream, a); break;
      case PMF_SIVM_L1: hipLaunchKernelGGL(k_laesa_pass<PMF_SIVM_L1>, grid, block, smem, c->stream, a); break;
      default: hipLaunchKernelGGL(k_laesa_pass<PMF_SIVM_COSINE>, grid, block, smem, c->stream, a); break;
    }
    stat_end(c, SITE_LAESA);
    HIPCHK(c, hipGetLastError());
  }
  return colsel_close(c, b, rounds.size(), wgs, C, nsel, nsel == 1 ? 1 : 0, (origin && nsel == 1) ? 1 : 0);
}

// GMAP.update_w (gmap.py:119-165, robust_map = False): nsel launches of k_gmap_pass -- round 0 the norms and the first argmax,
// round l measures against select[l - 1] and finds select[l] -- and the closing reduce.  Round 0 writes both state arrays whole.
int gmap_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int method, const SivmBufs& b) {
  int ppw = 0, wgs = 0;
  panel_partition((int)(ld / 64), PMF_CL_MAX_WGS, &ppw, &wgs);
  ColselArgs a = colsel_args(A, ld, R, C, b, ppw);
  const dim3 grid((unsigned)wgs), block(256);
  for (int l = 0; l < nsel; ++l) {
    colsel_flip(a, b, (size_t)l, wgs);
    a.first = l == 0;
    a.sel_pos = l - 1;
    const size_t smem = l == 0 ? 0 : (size_t)R * sizeof(float);
    stat_begin(c, SITE_GMAP);
    switch (method) {
      case PMF_GMAP_PCA: hipLaunchKernelGGL(k_gmap_pass<PMF_GMAP_PCA>, grid, block, smem, c->stream, a); break;
      case PMF_GMAP_AA: hipLaunchKernelGGL(k_gmap_pass<PMF_GMAP_AA>, grid, block, smem, c->stream, a); break;
      default: hipLaunchKernelGGL(k_gmap_pass<PMF_GMAP_NMF>, grid, block, smem, c->stream, a); break;
    }
    stat_end(c, SITE_GMAP);
    HIPCHK(c, hipGetLastError());
  }
  return colsel_close(c, b, (size_t)nsel, wgs, C, nsel, 0, 0);
}

}  // namespace
