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

int sivm_alloc(pmf_ctx* c) {
  if (c->dSvState) return PMF_OK;
  PMFCHK(dalloc(c, &c->dSvState, (size_t)3 * c->np));
  PMFCHK(dalloc(c, &c->dSvPart, (size_t)2 * PMF_CL_MAX_WGS));
  PMFCHK(dalloc(c, &c->dSvPartIdx, (size_t)2 * PMF_CL_MAX_WGS));
  PMFCHK(dalloc(c, &c->dSvSel, (size_t)c->KP));
  PMFCHK(dalloc(c, &c->dSvScal, 2));
  return PMF_OK;
}

// f(std::integral_constant<int, M>) for the runtime metric (or GMAP method) M = 0, 1, 2: the kernels take it as a template argument
template <class F>
void with_metric(int metric, F f) {
  switch (metric) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    default: f(std::integral_constant<int, 2>{}); break;
  }
}

// one k_sivm_pass over the matrix that `a` describes (a.m rows staged in LDS)
int sivm_launch_pass(pmf_ctx* c, const SivmArgs& a, int wgs, int metric) {
  stat_begin(c, SITE_SIVM);
  with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL(k_sivm_pass<decltype(M)::value>, dim3((unsigned)wgs), dim3(256), (size_t)a.m * sizeof(float), c->stream, a);
  });
  stat_end(c, SITE_SIVM);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// The rounds of update_w (sivm.py:145-201) as (plain, l, take_maxd, keep, sel_pos, last) per round: three plain rounds from
// candidate 0 ('fastmap') or one from the origin, then round l measures against select[l - 1] and finds select[l].
struct SivmRound { int plain, l, take_maxd, keep, sel_pos, last; };

std::vector<SivmRound> sivm_rounds(int nsel, bool origin) {
  std::vector<SivmRound> r;
  const int nplain = origin ? 1 : 3;
  for (int p = 0; p < nplain; ++p) r.push_back({1, 0, p == nplain - 1, origin ? 1 : 0, -1, 0});
  for (int l = 1; l < nsel; ++l) r.push_back({0, l, 0, 0, l - 1, 0});
  r.back().last = 1;
  return r;
}

// what the column-panel rounds write: the recurrence's state [3][ld], the two partials arrays of the argmax ([2][PMF_CL_MAX_WGS]
// each), (maxd, a) and the selection -- the resident buffers of the context (update_w) or temporaries of a pmf_sivm_select call
struct SivmBufs { double* state; double* part; int* pidx; double* scal; int* select; };

// A chain of column-panel launches on A [R rows][ld], candidates its C columns, as every driver of the family enqueues one
// (pmf_colsweep.h): a round's argmax is taken in the next launch's prologue, nothing is read by the host in between.
struct PanelChain { const SivmBufs& b; int wgs; size_t p; };   // the buffers, the workgroups of a launch, launches so far

// the partition, and what of the common argument block stays the same along the chain
PanelChain chain_begin(ColsweepArgs& a, const float* A, int64_t ld, int R, int C, const SivmBufs& b) {
  int wgs = 0;
  a.V = A; a.np = ld; a.m = R; a.n = C;
  a.npanels = (int)(ld / 64);
  panel_partition(a.npanels, PMF_CL_MAX_WGS, &a.panels_per_wg, &wgs);
  return {b, wgs, 0};
}

// the next launch reads the partials that the one before it wrote; returns its number in the chain
size_t chain_next(PanelChain& ch, ColsweepArgs& a) {
  const int out = (int)(ch.p & 1), in = out ^ 1;
  a.pscore_in = ch.b.part + in * PMF_CL_MAX_WGS; a.pidx_in = ch.b.pidx + in * PMF_CL_MAX_WGS;
  a.pscore_out = ch.b.part + out * PMF_CL_MAX_WGS; a.pidx_out = ch.b.pidx + out * PMF_CL_MAX_WGS;
  a.nprev = ch.p == 0 ? 0 : ch.wgs;
  return ch.p++;
}

// the reduce behind the last launch: select[sel_pos]; take_maxd: its score and the logarithm of it into scal[0], scal[1]
int chain_close(pmf_ctx* c, const PanelChain& ch, int C, int sel_pos, bool take_maxd, bool origin_first, double* scal) {
  const int last = (int)((ch.p - 1) & 1);
  hipLaunchKernelGGL(k_sivm_close, dim3(1), dim3(256), 0, c->stream, (const double*)(ch.b.part + last * PMF_CL_MAX_WGS),
                     (const int*)(ch.b.pidx + last * PMF_CL_MAX_WGS), ch.wgs, C, sel_pos, take_maxd ? 1 : 0, origin_first ? 1 : 0, ch.b.select, scal);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// k_sivm_pass: nsel + 2 ('fastmap') or nsel ('origin') launches back to back and the closing reduce
int sivm_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int metric, bool origin, const SivmBufs& b) {
  HIPCHK(c, hipMemsetAsync(b.state, 0, (size_t)3 * ld * sizeof(double), c->stream));
  SivmArgs a{};
  PanelChain ch = chain_begin(a, A, ld, R, C, b);
  a.dij = b.state; a.dsum = b.state + ld; a.dsq = b.state + 2 * ld;
  a.select = b.select; a.scal = b.scal;
  a.fixed_idx = origin ? -1 : 0;
  for (const SivmRound& r : sivm_rounds(nsel, origin)) {
    const size_t p = chain_next(ch, a);
    a.use_fixed = p == 0 || (origin && r.l == 1);
    a.sel_pos = r.sel_pos; a.take_maxd = r.l == 1; a.plain = r.plain; a.l = r.l;
    PMFCHK(sivm_launch_pass(c, a, ch.wgs, metric));
  }
  return chain_close(c, ch, C, nsel - 1, nsel == 1, origin && nsel == 1, b.scal);
}

// W = V[:, select] for the selection in dSvSel (SIVM, GREEDY)
int gather_selected_w(pmf_ctx* c) {
  const int64_t elems = c->mp * c->KP;
  hipLaunchKernelGGL(k_sivm_gather, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, c->stream, (const float*)c->dV, (int64_t)c->np,
                     (int)c->m, (int)c->n, c->k, c->KP, elems, (const int*)c->dSvSel, c->dW);
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  c->sv_have_select = true;
  return PMF_OK;
}

// the round drivers of the other two rules of a SIVM context (pmf_host_colsel.h)
int laesa_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int metric, bool origin, const SivmBufs& b);
int gmap_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int method, const SivmBufs& b);
// ... of SIVM and LAESA on CSC data (pmf_host_sivm_csc.h)
int sivm_csc_update_w(pmf_ctx* c);
int sivm_csc_wtv(pmf_ctx* c);
// ... and of SIVM_SGREEDY (pmf_host_sgreedy.h)
int sgreedy_panel_rounds(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int metric, bool origin, const SivmBufs& b);

// SIVM.update_w (sivm.py:145-201), LAESA.update_w (laesa.py:63-82) or GMAP.update_w (gmap.py:119-165) by the context's rule, or
// SIVM_SGREEDY.update_w (sivm_sgreedy.py:96-133) under "sivm_sgreedy":
// the rounds on the resident V and buffers, then the gather
int sivm_update_w(pmf_ctx* c) {
  if (c->v_csc) return sivm_csc_update_w(c);
  if (c->sv_gsat) return fail(c, PMF_EINVAL, "SIVM_GSAT: no W step of its own (pmf_gsat_walk and pmf_gsat_probe_vec move the vertices)");
  PMFCHK(sivm_alloc(c));
  const SivmBufs b{c->dSvState, c->dSvPart, c->dSvPartIdx, c->dSvScal, c->dSvSel};
  if (c->sv_sgreedy) PMFCHK(sgreedy_panel_rounds(c, c->dV, c->np, (int)c->m, (int)c->n, c->k, c->sv_metric, c->sv_init == 1, b));
  else if (c->sv_rule == 1) PMFCHK(laesa_panel_rounds(c, c->dV, c->np, (int)c->m, (int)c->n, c->k, c->sv_metric, c->sv_init == 1, b));
  else if (c->sv_rule == 2) PMFCHK(gmap_panel_rounds(c, c->dV, c->np, (int)c->m, (int)c->n, c->k, c->sv_gmap_method, b));
  else PMFCHK(sivm_panel_rounds(c, c->dV, c->np, (int)c->m, (int)c->n, c->k, c->sv_metric, c->sv_init == 1, b));
  return gather_selected_w(c);
}

// ---- pmf_sivm_select: the selection alone, among the columns of the resident V or among its rows (SIVM_CUR) --------------------
// the column-panel rounds with state and partials as temporaries of the call
int sivm_select_panels(pmf_ctx* c, const float* A, int64_t ld, int R, int C, int nsel, int metric, bool origin, int* dsel, DevTemps& tmp) {
  SivmBufs b{nullptr, nullptr, nullptr, nullptr, dsel};
  PMFCHK(talloc(c, tmp, &b.state, (size_t)3 * ld));
  PMFCHK(talloc(c, tmp, &b.part, (size_t)2 * PMF_CL_MAX_WGS));
  PMFCHK(talloc(c, tmp, &b.pidx, (size_t)2 * PMF_CL_MAX_WGS));
  PMFCHK(talloc(c, tmp, &b.scal, 2));
  return sivm_panel_rounds(c, A, ld, R, C, nsel, metric, origin, b);
}

template <int METRIC>
void sivm_launch_rowdist(pmf_ctx* c, const SivmRowArgs& a) {
  hipLaunchKernelGGL(k_sivm_rowdist<METRIC>, dim3((unsigned)a.slabs, (unsigned)((a.C + PMF_SIVM_ROWS_WG - 1) / PMF_SIVM_ROWS_WG)), dim3(256), 0,
                     c->stream, a);
}

// the long-sample pass on A [C rows][ld], candidates its rows, R valid columns: two launches per round, enqueued back to back
int sivm_select_rows(pmf_ctx* c, const float* A, int64_t ld, int C, int R, int nsel, int metric, bool origin, int* dsel, DevTemps& tmp) {
  const int slabs = (R + PMF_SIVM_SLAB - 1) / PMF_SIVM_SLAB;
  const int Cs = (int)round_up(C, PMF_SIVM_ROWS_WG);
  const int64_t blk = (int64_t)slabs * Cs;
  double *state = nullptr, *part = nullptr, *xpart = nullptr, *scal = nullptr;
  int* cur = nullptr;
  PMFCHK(talloc(c, tmp, &state, (size_t)3 * Cs));
  PMFCHK(talloc(c, tmp, &part, (size_t)(metric == PMF_SIVM_COSINE ? 2 : 1) * blk));
  PMFCHK(talloc(c, tmp, &xpart, (size_t)slabs));
  PMFCHK(talloc(c, tmp, &scal, 2));
  PMFCHK(talloc(c, tmp, &cur, 1));
  HIPCHK(c, hipMemsetAsync(state, 0, (size_t)3 * Cs * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(cur, origin ? 0xff : 0, sizeof(int), c->stream));      // -1 or 0
  SivmRowArgs d{};
  d.A = A; d.ld = ld; d.cur = cur; d.part = part; d.xpart = xpart; d.C = C; d.R = R; d.Cs = Cs; d.slabs = slabs;
  SivmRowStepArgs s{};
  s.part = part; s.xpart = xpart; s.dij = state; s.dsum = state + Cs; s.dsq = state + 2 * Cs; s.cur = cur; s.select = dsel; s.scal = scal;
  s.C = C; s.Cs = Cs; s.slabs = slabs; s.metric = metric;
  s.tpr = 1;                                           // threads per row of the slab sum: all 256 busy while C is small
  while (s.tpr < 64 && 2 * s.tpr * C <= 256 && s.tpr < slabs) s.tpr *= 2;
  if (c->profile && c->stat.site == SITE_SIVM_ROWS) {
    static const char* const names[3] = {"k_sivm_rowdist<l2>+k_sivm_rowstep", "k_sivm_rowdist<l1>+k_sivm_rowstep", "k_sivm_rowdist<cosine>+k_sivm_rowstep"};
    c->stat.name = names[metric];
    c->stat.flops = c->stat.exec_flops = (metric == PMF_SIVM_COSINE ? 4.0 : 3.0) * (double)C * (double)R;
    // A once, x once per row block; the partials written and read; the state read and written
    c->stat.bytes = 4.0 * (double)C * (double)R + 4.0 * (double)R * (double)(Cs / PMF_SIVM_ROWS_WG) +
                    16.0 * (double)blk * (metric == PMF_SIVM_COSINE ? 2.0 : 1.0) + 48.0 * (double)C;
  }
  for (const SivmRound& r : sivm_rounds(nsel, origin)) {
    stat_begin(c, SITE_SIVM_ROWS);
    with_metric(metric, [&](auto M) { sivm_launch_rowdist<decltype(M)::value>(c, d); });
    HIPCHK(c, hipGetLastError());
    s.plain = r.plain; s.l = r.l; s.take_maxd = r.take_maxd; s.keep_cur = r.keep; s.sel_pos = r.sel_pos;
    s.last_pos = r.last ? nsel - 1 : -1;
    hipLaunchKernelGGL(k_sivm_rowstep, dim3(1), dim3(256), 0, c->stream, s);
    stat_end(c, SITE_SIVM_ROWS);
    HIPCHK(c, hipGetLastError());
  }
  return PMF_OK;
}

// nsel indices in selection order into dsel (device): among the columns of V, or (trans) among its rows.  path 0: by shape
// (DESIGN.md 3.17); 1 / 2: k_sivm_pass / the long-sample pass forced, on a transposed copy where the layout needs one.
// Synchronises at the end.  Always SIVM's rule, whatever "sivm_rule" the context carries (SIVM_CUR depends on it).
bool sivm_rows_path(const pmf_ctx* c, bool trans, int path) {
  return path == 0 ? (trans == (c->m <= PMF_SIVM_MAX_M)) : path == 2;
}

// the transposed view of the resident V as a matrix of its own, [np][mp], a temporary of the call
int transposed_view(pmf_ctx* c, DevTemps& tmp, const float** A, int64_t* ld) {
  float* AT = nullptr;
  PMFCHK(talloc(c, tmp, &AT, (size_t)c->np * c->mp));
  hipLaunchKernelGGL(k_greedy_transpose, dim3((unsigned)(c->mp / 64), (unsigned)(c->np / 64)), dim3(256), 0, c->stream, (const float*)c->dV,
                     (int64_t)c->np, AT, (int64_t)c->mp);
  HIPCHK(c, hipGetLastError());
  *A = AT;
  *ld = c->mp;
  return PMF_OK;
}

int sivm_select(pmf_ctx* c, bool trans, int nsel, int metric, bool origin, int path, int* dsel) {
  const int64_t C = trans ? c->m : c->n, R = trans ? c->n : c->m;
  const bool rows_path = sivm_rows_path(c, trans, path);
  DevTemps tmp;
  const float* A = c->dV;
  int64_t ld = c->np;
  if (rows_path != trans) PMFCHK(transposed_view(c, tmp, &A, &ld));   // the pass wants the other layout
  if (rows_path) PMFCHK(sivm_select_rows(c, A, ld, (int)C, (int)R, nsel, metric, origin, dsel, tmp));
  else PMFCHK(sivm_select_panels(c, A, ld, (int)R, (int)C, nsel, metric, origin, dsel, tmp));
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  return PMF_OK;
}

// pmf_sivm_select: the arguments checked before anything is touched, the selection, read back
int sivm_select_host(pmf_ctx* c, bool trans, int nsel, int metric, int init, int path, int32_t* select) {
  if (c->v_csr || c->v_csc || !c->dV) return fail(c, PMF_EINVAL, "pmf_sivm_select: dense resident data only");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_sivm_select: one rank only in this build");
  if (nsel < 1 || nsel > 64) return fail(c, PMF_EINVAL, "pmf_sivm_select: 1 <= nsel <= 64");
  if (metric < 0 || metric > 2) return fail(c, PMF_EINVAL, "pmf_sivm_select: metric 0 (l2), 1 (l1) or 2 (cosine)");
  if (init != 0 && init != 1) return fail(c, PMF_EINVAL, "pmf_sivm_select: init 0 (fastmap) or 1 (origin)");
  if (path < 0 || path > 2) return fail(c, PMF_EINVAL, "pmf_sivm_select: path 0 (by shape), 1 (column panels) or 2 (long samples)");
  if (std::min<int64_t>(c->m, c->n) > PMF_SIVM_MAX_M) return fail(c, PMF_EINVAL, "pmf_sivm_select: min(rows, cols) > 16384 is not supported by this build");
  if (sivm_rows_path(c, trans, path) ? (trans ? c->m : c->n) > PMF_SIVM_ROW_MAX_C : (trans ? c->n : c->m) > PMF_SIVM_MAX_M)
    return fail(c, PMF_EINVAL, path == 2 ? "pmf_sivm_select: the long-sample pass takes at most 16384 candidates"
                                         : "pmf_sivm_select: the column-panel pass takes samples of dimension <= 16384");
  DevTemps tmp;
  int* dsel = nullptr;
  PMFCHK(talloc(c, tmp, &dsel, 64));
  PMFCHK(sivm_select(c, trans, nsel, metric, init == 1, path, dsel));
  HIPCHK(c, hipMemcpyAsync(select, dsel, (size_t)nsel * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

// AA.update_h (aa.py:93-111): one simplex-constrained QP per column, as rounds of non-negative QPs (pmf_sivm.h)
int sivm_update_h(pmf_ctx* c) {
  if (c->v_csc) PMFCHK(sivm_csc_wtv(c));         // dPS = (W^T V | ...) from the stored entries
  else PMFCHK(ensure_ps(c));                     // dPS = (W^T V | W^T W), float32
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

}  // namespace
