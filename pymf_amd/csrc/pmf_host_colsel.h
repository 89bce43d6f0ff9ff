// pmf_host_colsel.h -- LAESA and GMAP: the round drivers of the two lighter selection rules of a SIVM context (kernels: pmf_colsel.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// a chain of either rule (PanelChain, pmf_host_sivm.h) and what its launches share: the state (>= 2 ld doubles) and SIVM's buffers
PanelChain colsel_begin(ColselArgs& a, const float* A, int64_t ld, int R, int C, const SivmBufs& b) {
  a.st0 = b.state; a.st1 = b.state + ld;
  a.select = b.select; a.scal = b.scal;
  return chain_begin(a, A, ld, R, C, b);
}

// one k_laesa_pass over the matrix that `a` describes (outside the profile's site: SIVM_SGREEDY's plain rounds are not LAESA's)
void laesa_launch_pass(pmf_ctx* c, const ColselArgs& a, int wgs, int metric) {
  with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL(k_laesa_pass<decltype(M)::value>, dim3((unsigned)wgs), dim3(256), (size_t)a.m * sizeof(float), c->stream, a);
  });
}

// LAESA.update_w (laesa.py:63-82) on A [R rows][ld], candidates its C columns: the rounds of sivm_rounds -- nsel + 2 ('fastmap')
// or nsel ('origin') launches of k_laesa_pass back to back -- and the closing reduce.  The state needs no clearing: the first
// recurrence round writes it whole.
int laesa_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int metric, bool origin, const SivmBufs& b) {
  ColselArgs a{};
  PanelChain ch = colsel_begin(a, A, ld, R, C, b);
  a.fixed_idx = origin ? -1 : 0;
  for (const SivmRound& r : sivm_rounds(nsel, origin)) {
    const size_t p = chain_next(ch, a);
    a.use_fixed = p == 0 || (origin && r.l == 1);
    a.sel_pos = r.sel_pos; a.take_maxd = r.l == 1; a.plain = r.plain; a.first = r.l == 1;
    stat_begin(c, SITE_LAESA);
    laesa_launch_pass(c, a, ch.wgs, metric);
    stat_end(c, SITE_LAESA);
    HIPCHK(c, hipGetLastError());
  }
  return chain_close(c, ch, C, nsel - 1, nsel == 1, origin && nsel == 1, b.scal);
}

// GMAP.update_w (gmap.py:119-165, robust_map = False): nsel launches of k_gmap_pass -- round 0 the norms and the first argmax,
// round l measures against select[l - 1] and finds select[l] -- and the closing reduce.  Round 0 writes both state arrays whole.
int gmap_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int method, const SivmBufs& b) {
  ColselArgs a{};
  PanelChain ch = colsel_begin(a, A, ld, R, C, b);
  for (int l = 0; l < nsel; ++l) {
    chain_next(ch, a);
    a.first = l == 0;
    a.sel_pos = l - 1;
    const size_t smem = l == 0 ? 0 : (size_t)R * sizeof(float);
    stat_begin(c, SITE_GMAP);
    with_metric(method, [&](auto M) {
      hipLaunchKernelGGL(k_gmap_pass<decltype(M)::value>, dim3((unsigned)ch.wgs), dim3(256), smem, c->stream, a);
    });
    stat_end(c, SITE_GMAP);
    HIPCHK(c, hipGetLastError());
  }
  return chain_close(c, ch, C, nsel - 1, false, false, b.scal);
}

}  // namespace
