// pmf_host_gsat.h -- SIVM_GSAT: the start of the walk's state and the batch loop of a SIVM context under "sivm_gsat" (kernels: pmf_gsat.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

constexpr int PMF_GSAT_TAB = PMF_GSAT_MAX_K * PMF_GSAT_MAX_K;   // dGsTab: the table, then the last probe's distances [64], then V

int gsat_alloc(pmf_ctx* c) {
  if (c->dGsW) return PMF_OK;
  PMFCHK(dalloc(c, &c->dGsW, (size_t)c->k * c->m));
  PMFCHK(dalloc(c, &c->dGsTab, (size_t)PMF_GSAT_TAB + PMF_GSAT_MAX_K + 2));
  PMFCHK(dalloc(c, &c->dGsProbe, (size_t)PMF_GSAT_BATCH * (PMF_GSAT_MAX_K + 1)));
  PMFCHK(dalloc(c, &c->dGsCtl, 2));
  PMFCHK(sivm_alloc(c));                         // dSvSel: `select` lives where pmf_sivm_get_select reads it
  return PMF_OK;
}

// what stays the same through a call
GsatArgs gsat_args(pmf_ctx* c) {
  GsatArgs a{};
  a.V = c->dV; a.np = c->np; a.m = (int)c->m; a.k = c->k; a.KP = c->KP;
  a.Wg = c->dGsW; a.W = c->dW; a.Dt = c->dGsTab; a.last = c->dGsTab + PMF_GSAT_TAB; a.Vcur = c->dGsTab + PMF_GSAT_TAB + PMF_GSAT_MAX_K;
  a.select = c->dSvSel; a.pvol = c->dGsProbe; a.pdist = c->dGsProbe + PMF_GSAT_BATCH; a.ctl = c->dGsCtl;
  a.l1 = c->sv_metric == 1 ? 1 : 0;
  return a;
}

int gsat_usable(pmf_ctx* c, const char* who) {
  if (c->algo != PMF_ALGO_SIVM || !c->sv_gsat) return fail(c, PMF_EINVAL, std::string(who) + ": SIVM contexts under sivm_gsat only");
  if (c->sv_metric == 2) return fail(c, PMF_EINVAL, std::string(who) + ": sivm_metric 0 (l2) or 1 (l1): the reference's cosine distance cannot take num_bases vertices");
  return PMF_OK;
}

// the walk's state from the context's W and the caller's `select`: the image, the table, V = cmdet(D) (sivm_gsat.py:84-88)
int gsat_start(pmf_ctx* c, const int32_t* select) {
  if (c->v_csr || c->v_csc || !c->dV) return fail(c, PMF_EINVAL, "pmf_gsat_start: dense resident data only");
  PMFCHK(gsat_alloc(c));
  c->gs_started = false;
  HIPCHK(c, hipMemcpyAsync(c->dSvSel, select, (size_t)c->k * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  GsatArgs a = gsat_args(c);
  hipLaunchKernelGGL(k_gsat_take_w, dim3((unsigned)c->k), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_gsat_table, dim3((unsigned)c->k), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_gsat_volume, dim3(1), dim3(64), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(a.last, 0, PMF_GSAT_MAX_K * sizeof(double), c->stream));
  HIPCHK(c, hipMemcpyAsync(&c->gs_V, a.Vcur, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));    // (`select` is the caller's memory)
  c->gs_log.clear();
  c->gs_started = true;
  c->sv_have_select = true;
  return PMF_OK;
}

// n probes in order -- data columns didx (device) or, vec given, that one vector --: launch pairs on the probes behind the last
// accepted one until each batch is used up; one 4-byte read per pair.  dslots [n] (device) takes the verdicts.
int gsat_run(pmf_ctx* c, const int64_t* didx, const float* dvec, int64_t n, int* dslots) {
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};      // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gsat_probe), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)gsat_probe_smem(PMF_GSAT_MAX_K)));
    attr_done = true;
  }
  DevTemps tmp;
  double* dlog = nullptr;
  PMFCHK(talloc(c, tmp, &dlog, (size_t)n));
  HIPCHK(c, hipMemsetAsync(c->dGsCtl, 0, 2 * sizeof(int), c->stream));
  GsatArgs a = gsat_args(c);
  a.vec = dvec; a.log = dlog;
  const size_t smem = gsat_probe_smem(c->k);
  for (int64_t base = 0; base < n; base += PMF_GSAT_BATCH) {
    const int nb = (int)std::min<int64_t>(PMF_GSAT_BATCH, n - base);
    for (int off = 0; off < nb;) {
      a.idx = didx ? didx + base + off : nullptr;
      a.slots = dslots + base + off;
      a.count = nb - off;
      hipLaunchKernelGGL(k_gsat_probe, dim3((unsigned)a.count), dim3(256), smem, c->stream, a);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(k_gsat_commit, dim3(1), dim3(256), 0, c->stream, a);
      HIPCHK(c, hipGetLastError());
      int pos = 0;
      HIPCHK(c, hipMemcpyAsync(&pos, c->dGsCtl, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (pos < 0 || pos > a.count) return fail(c, PMF_ENUMERIC, "SIVM_GSAT: the commit reported a position outside its launch");
      off += pos < a.count ? pos + 1 : a.count;
    }
  }
  // the accepted volumes onto the reference's _v ([the volume before the first swap, the accepted ones ...]), V, the context's W
  int nacc = 0;
  HIPCHK(c, hipMemcpyAsync(&nacc, c->dGsCtl + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (nacc < 0 || nacc > n) return fail(c, PMF_ENUMERIC, "SIVM_GSAT: more accepted probes than probes");
  if (nacc > 0) {
    std::vector<double> acc((size_t)nacc);
    HIPCHK(c, hipMemcpyAsync(acc.data(), dlog, (size_t)nacc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->gs_log.empty()) c->gs_log.push_back(c->gs_V);
    c->gs_log.insert(c->gs_log.end(), acc.begin(), acc.end());
    c->gs_V = acc.back();
    w_replaced(c, false);
  }
  return PMF_OK;
}

int gsat_ready(pmf_ctx* c, const char* who) {
  PMFCHK(gsat_usable(c, who));
  if (!c->gs_started) return fail(c, PMF_EINVAL, std::string(who) + ": the walk has no state for the current W (pmf_gsat_start)");
  return PMF_OK;
}

int gsat_walk(pmf_ctx* c, const int64_t* idx, int64_t n, int32_t* slots_out) {
  PMFCHK(gsat_ready(c, "pmf_gsat_walk"));
  if (n < 0 || n > (int64_t)1 << 28) return fail(c, PMF_EINVAL, "pmf_gsat_walk: 0 <= n <= 2^28 probes");
  for (int64_t i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= c->n) return fail(c, PMF_EINVAL, "pmf_gsat_walk: a probe index outside [0, num_samples)");
  if (n == 0) return PMF_OK;
  DevTemps tmp;
  int64_t* didx = nullptr;
  int* dslots = nullptr;
  PMFCHK(talloc(c, tmp, &didx, (size_t)n));
  PMFCHK(talloc(c, tmp, &dslots, (size_t)n));
  HIPCHK(c, hipMemcpyAsync(didx, idx, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  PMFCHK(gsat_run(c, didx, nullptr, n, dslots));
  HIPCHK(c, hipMemcpyAsync(slots_out, dslots, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

int gsat_probe_vec(pmf_ctx* c, const float* vec, int32_t* slot_out) {
  PMFCHK(gsat_ready(c, "pmf_gsat_probe_vec"));
  DevTemps tmp;
  float* dvec = nullptr;
  int* dslot = nullptr;
  PMFCHK(talloc(c, tmp, &dvec, (size_t)c->m));
  PMFCHK(talloc(c, tmp, &dslot, 1));
  HIPCHK(c, hipMemcpyAsync(dvec, vec, (size_t)c->m * sizeof(float), hipMemcpyHostToDevice, c->stream));
  PMFCHK(gsat_run(c, nullptr, dvec, 1, dslot));
  HIPCHK(c, hipMemcpyAsync(slot_out, dslot, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

// the reference's D as it leaves it: D[:k, :k] the table, row and column k the last probe's distances, D[k, k] = 0
int gsat_get_d(pmf_ctx* c, double* D) {
  PMFCHK(gsat_ready(c, "pmf_gsat_get_d"));
  std::vector<double> t((size_t)PMF_GSAT_TAB + PMF_GSAT_MAX_K);
  HIPCHK(c, hipMemcpyAsync(t.data(), c->dGsTab, t.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int k = c->k, T = k + 1;
  for (int i = 0; i < T; ++i)
    for (int j = 0; j < T; ++j)
      D[i * T + j] = (i < k && j < k) ? t[(size_t)i * PMF_GSAT_MAX_K + j] : (i == j) ? 0.0 : t[(size_t)PMF_GSAT_TAB + std::min(i, j)];
  return PMF_OK;
}

}  // namespace
