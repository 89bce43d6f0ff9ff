// pmf_host_sivm_csc.h -- SIVM and LAESA on CSC data: the checked upload, the selection rounds, the gather of W and the W^T V block
// of the H step (kernels: pmf_sivm_csc.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
//
// State (pmf_ctx): the CSC arrays of V in dIndptr [np + 1], dIndices, dVals (the fields that hold the CSR arrays of an SNMF or NMF
// context) under v_csc; no dense V: dV is released by the upload, so every dense-only entry point finds no data.  Selection
// state, partials, select and the H step's buffers are the dense path's.
#pragma once

namespace {

// The team of k_sivm_csc_pass by the mean stored entries per column: a team takes TEAM entries of its column per trip, so the
// mean column should cost a few trips at the most and not leave most of the team idle.  Up to 8 entries: 4 lanes (<= 2 trips);
// up to 48: 16 lanes (<= 3 trips); beyond: a whole wave.
constexpr double PMF_CSC_TEAM4_MAX_MEAN = 8.0;
constexpr double PMF_CSC_TEAM16_MAX_MEAN = 48.0;

int sivm_csc_team(const pmf_ctx* c) {
  if (c->opt_sivm_csc_team) return c->opt_sivm_csc_team;
  const double mean = (double)c->nnz / (double)c->n;
  return mean <= PMF_CSC_TEAM4_MAX_MEAN ? 4 : mean <= PMF_CSC_TEAM16_MAX_MEAN ? 16 : 64;
}

// pmf_path_name while CSC data is resident: the team that the next W step runs with
void sivm_csc_name_path(pmf_ctx* c) { c->path = "sivm_csc_teams<" + std::to_string(sivm_csc_team(c)) + ">"; }

// CSC arrays of an m x n matrix as pmf_set_v_csc_f32 takes them: null, or what is wrong with them (host only)
const char* csc_check(int64_t m, int64_t n, const int64_t* indptr, const int32_t* indices, int64_t nnz) {
  if (indptr[0] != 0 || indptr[n] != nnz) return "indptr[0] must be 0 and indptr[n] must be nnz";
  for (int64_t c = 0; c < n; ++c)
    if (indptr[c + 1] < indptr[c]) return "indptr must not decrease";
  for (int64_t c = 0; c < n; ++c)
    for (int64_t e = indptr[c]; e < indptr[c + 1]; ++e) {
      if (indices[e] < 0 || indices[e] >= m) return "row index out of range";
      if (e > indptr[c] && indices[e] <= indices[e - 1]) return "row indices must ascend within a column, without duplicates";
    }
  return nullptr;
}

// dense data came back to the context (or none is left): the CSC arrays go
int sivm_csc_left(pmf_ctx* c) {
  if (!c->v_csc) return PMF_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dIndptr));
  PMFCHK(dfree(c, &c->dIndices));
  PMFCHK(dfree(c, &c->dVals));
  c->v_csc = false; c->nnz = 0;
  c->path = "sivm_panels";
  return PMF_OK;
}

// the rules that have no CSC pass
const char* sivm_csc_refused_rule(const pmf_ctx* c) {
  if (c->sv_gsat) return "SIVM_GSAT";
  if (c->sv_sgreedy) return "SIVM_SGREEDY";
  if (c->sv_rule == 2) return "GMAP";
  return nullptr;
}

int sivm_csc_set_v(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz) {
  if (c->algo != PMF_ALGO_SIVM) return fail(c, PMF_EINVAL, "pmf_set_v_csc_f32: SIVM contexts under the rules SIVM and LAESA only");
  if (const char* rule = sivm_csc_refused_rule(c)) return fail(c, PMF_EINVAL, std::string("pmf_set_v_csc_f32: ") + rule + " takes dense data only");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_set_v_csc_f32: one rank only in this build");
  if (const char* why = csc_check(c->m, c->n, indptr, indices, nnz)) return fail(c, PMF_EINVAL, std::string("pmf_set_v_csc_f32: ") + why);
  std::vector<int64_t> ip((size_t)c->np + 1);
  for (int64_t q = 0; q <= c->np; ++q) ip[(size_t)q] = indptr[std::min<int64_t>(q, c->n)];   // (columns >= n: empty)
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dV));                            // a CSC upload replaces dense data
  PMFCHK(dgrow(c, &c->dIndptr, (size_t)c->np + 1));
  PMFCHK(dgrow(c, &c->dIndices, (size_t)nnz));
  PMFCHK(dgrow(c, &c->dVals, (size_t)nnz));
  HIPCHK(c, hipMemcpyAsync(c->dIndptr, ip.data(), ip.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  if (nnz) {
    HIPCHK(c, hipMemcpyAsync(c->dIndices, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dVals, vals, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));          // (ip leaves scope; the caller's arrays are copied)
  c->nnz = nnz; c->have_v = true; c->v_csr = false; c->csr_dense = false; c->v_csc = true;
  v_replaced(c);
  sivm_csc_name_path(c);
  return PMF_OK;
}

template <int METRIC, int RULE, int TEAM>
int sivm_csc_launch(pmf_ctx* c, const SivmCscArgs& a, int wgs) {
  const size_t smem = (size_t)a.m * sizeof(float);
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};     // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {                                    // (m = 16384: 64 KiB of dynamic LDS beside the kernel's static words)
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sivm_csc_pass<METRIC, RULE, TEAM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(PMF_SIVM_MAX_M * sizeof(float))));
    attr_done = true;
  }
  hipLaunchKernelGGL((k_sivm_csc_pass<METRIC, RULE, TEAM>), dim3((unsigned)wgs), dim3(256), smem, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

template <int METRIC, int RULE>
int sivm_csc_launch_team(pmf_ctx* c, const SivmCscArgs& a, int wgs, int team) {
  switch (team) {
    case 4: return sivm_csc_launch<METRIC, RULE, 4>(c, a, wgs);
    case 16: return sivm_csc_launch<METRIC, RULE, 16>(c, a, wgs);
    default: return sivm_csc_launch<METRIC, RULE, 64>(c, a, wgs);
  }
}

int sivm_csc_launch_pass(pmf_ctx* c, const SivmCscArgs& a, int wgs, int metric, int rule, int team) {
  int rc = PMF_OK;
  stat_begin(c, rule ? SITE_LAESA : SITE_SIVM);
  with_metric(metric, [&](auto M) {
    rc = rule ? sivm_csc_launch_team<decltype(M)::value, PMF_CSC_RULE_LAESA>(c, a, wgs, team)
              : sivm_csc_launch_team<decltype(M)::value, PMF_CSC_RULE_SIVM>(c, a, wgs, team);
  });
  stat_end(c, rule ? SITE_LAESA : SITE_SIVM);
  return rc;
}

// SIVM.update_w / LAESA.update_w on the resident CSC data: the rounds of sivm_rounds on k_sivm_csc_pass, back to back, the closing
// reduce, the gather of W.  The partition is chain_begin's: contiguous ranges of 64-column panels.
int sivm_csc_update_w(pmf_ctx* c) {
  if (const char* rule = sivm_csc_refused_rule(c))
    return fail(c, PMF_EINVAL, std::string(rule) + ": dense data only (the context holds CSC data: SIVM and LAESA select from it)");
  PMFCHK(sivm_alloc(c));
  const SivmBufs b{c->dSvState, c->dSvPart, c->dSvPartIdx, c->dSvScal, c->dSvSel};
  const bool origin = c->sv_init == 1, laesa = c->sv_rule == 1;
  const int nsel = c->k, team = sivm_csc_team(c);
  const int64_t ld = c->np;
  if (!laesa) HIPCHK(c, hipMemsetAsync(b.state, 0, (size_t)3 * ld * sizeof(double), c->stream));   // (LAESA's first round writes dmin whole)
  SivmCscArgs a{};
  PanelChain ch = chain_begin(a, nullptr, ld, (int)c->m, (int)c->n, b);
  a.indptr = c->dIndptr; a.indices = c->dIndices; a.vals = c->dVals;
  a.st0 = b.state; a.st1 = b.state + ld; a.st2 = b.state + 2 * ld;
  a.select = b.select; a.scal = b.scal;
  a.fixed_idx = origin ? -1 : 0;
  if (c->profile && (c->stat.site == SITE_SIVM || c->stat.site == SITE_LAESA)) {
    static const char* const names[2][3] = {{"k_sivm_csc_pass<l2>", "k_sivm_csc_pass<l1>", "k_sivm_csc_pass<cosine>"},
                                            {"k_sivm_csc_pass<l2,laesa>", "k_sivm_csc_pass<l1,laesa>", "k_sivm_csc_pass<cosine,laesa>"}};
    c->stat.name = names[laesa ? 1 : 0][c->sv_metric];
    c->stat.flops = c->stat.exec_flops = (c->sv_metric == PMF_SIVM_COSINE ? 4.0 : 5.0) * (double)c->nnz;
    // the entries (value and row id) once; per column its indptr words and the score; the state read and written (SIVM: three arrays)
    c->stat.bytes = 8.0 * (double)c->nnz + 24.0 * (double)c->n + (laesa ? 16.0 : 48.0) * (double)c->n;
  }
  for (const SivmRound& r : sivm_rounds(nsel, origin)) {
    const size_t p = chain_next(ch, a);
    a.use_fixed = p == 0 || (origin && r.l == 1);
    a.sel_pos = r.sel_pos; a.take_maxd = r.l == 1; a.plain = r.plain; a.first = r.l == 1; a.l = r.l;
    PMFCHK(sivm_csc_launch_pass(c, a, ch.wgs, c->sv_metric, c->sv_rule, team));
  }
  PMFCHK(chain_close(c, ch, (int)c->n, nsel - 1, nsel == 1, origin && nsel == 1, b.scal));
  HIPCHK(c, hipMemsetAsync(c->dW, 0, (size_t)c->mp * c->KP * sizeof(float), c->stream));
  hipLaunchKernelGGL(k_sivm_csc_gather, dim3((unsigned)c->k), dim3(256), 0, c->stream, (const int64_t*)c->dIndptr, (const int32_t*)c->dIndices,
                     (const float*)c->dVals, (int)c->n, c->KP, (const int*)c->dSvSel, c->dW);
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  c->sv_have_select = true;
  return PMF_OK;
}

// the W^T V block of dPS from the stored entries (the H step reads nothing else of dPS: W^T W is k_sivm_hessian's, in float64)
int sivm_csc_wtv(pmf_ctx* c) {
  const int64_t ldp = (int64_t)c->np + c->KP;
  const dim3 grid((unsigned)(c->np / 64));
#define PMF_CSC_WTV(NT_)                                                                                                                  \
  hipLaunchKernelGGL((k_csc_wtv<NT_>), grid, dim3(256), 0, c->stream, (const int64_t*)c->dIndptr, (const int32_t*)c->dIndices, \
                     (const float*)c->dVals, (const float*)c->dW, c->dPS, ldp)
  switch (c->NT) {
    case 1: PMF_CSC_WTV(1); break;
    case 2: PMF_CSC_WTV(2); break;
    case 4: PMF_CSC_WTV(4); break;
    default: return fail(c, PMF_EINVAL, "SIVM on CSC data: num_bases > 64 is not supported by this build");
  }
#undef PMF_CSC_WTV
  HIPCHK(c, hipGetLastError());
  c->ps_valid = false;                                 // (the W^T W block of dPS is not formed)
  return PMF_OK;
}

}  // namespace
