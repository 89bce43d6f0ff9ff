// pmf_host_cluster.h -- Kmeans / Cmeans: the one-pass iteration over column panels (kernels: pmf_cluster.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// The reference's iteration is update_w, then update_h (nmf.py:183-187): W from the assignment / memberships at hand, then
// the new ones.  One launch of k_cluster_pass assigns with the current W and leaves the sums that the NEXT update_w divides
// (cl_sums_valid); an update_w that no pass preceded (H from the caller, Cmeans' random H0) forms the sums alone first.
inline bool is_cluster(const pmf_ctx* c) { return c->algo == PMF_ALGO_KMEANS || c->algo == PMF_ALGO_CMEANS; }
// CSR data is resident on the context: the steps and the error of pmf_host_cluster_csr.h (further down the include order)
inline bool cluster_csr(const pmf_ctx* c) { return is_cluster(c) && c->v_csr; }
int cluster_csr_update_w(pmf_ctx* c);
int cluster_csr_update_h(pmf_ctx* c);
int cluster_csr_error(pmf_ctx* c, double* out);

// contiguous ranges of 64-column panels over at most `cap` workgroups: the panels each owns and how many there are
// (k_cluster_pass, k_sivm_pass, k_aa_price, k_greedy_pass)
void panel_partition(int npanels, int cap, int* ppw, int* wgs) {
  const int want = std::min(npanels, cap);
  *ppw = (npanels + want - 1) / want;
  *wgs = (npanels + *ppw - 1) / *ppw;
}

int cluster_alloc(pmf_ctx* c) {
  if (c->dClNum) return PMF_OK;                    // (released while CSR data is resident: cluster_csr_set_v)
  // a slab of mp x KP floats per workgroup: at most PMF_CL_MAX_WGS of them and 2 GiB in all (few, tall slabs when m >> n)
  const int64_t by_mem = std::max<int64_t>(1, ((int64_t)1 << 31) / (c->mp * c->KP * (int64_t)sizeof(float)));
  panel_partition(c->np / 64, (int)std::min<int64_t>(PMF_CL_MAX_WGS, by_mem), &c->cl_ppw, &c->cl_wgs);
  PMFCHK(dalloc(c, &c->dClNum, (size_t)c->cl_wgs * c->mp * c->KP));
  if (!c->dClDen) PMFCHK(dalloc(c, &c->dClDen, (size_t)c->cl_wgs * c->KP));
  if (!c->dClErr) PMFCHK(dalloc(c, &c->dClErr, (size_t)c->cl_wgs * 2));
  if (!c->dClWn) PMFCHK(dalloc(c, &c->dClWn, (size_t)c->KP));
  if (!c->dClTot) PMFCHK(dalloc(c, &c->dClTot, (size_t)c->KP + 2));
  if (!c->dClMu) PMFCHK(dalloc(c, &c->dClMu, (size_t)c->mp));
  if (!c->dClAsg) PMFCHK(dalloc(c, &c->dClAsg, (size_t)c->np));
  return PMF_OK;
}

template <int NT>
int cluster_launch_t(pmf_ctx* c, const ClusterArgs& a) {
  if (c->algo == PMF_ALGO_KMEANS)
    hipLaunchKernelGGL((k_cluster_pass<NT, PMF_CL_KMEANS>), dim3((unsigned)c->cl_wgs), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL((k_cluster_pass<NT, PMF_CL_CMEANS>), dim3((unsigned)c->cl_wgs), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// assign: the H step (assignment / memberships from the current W) with the sums; otherwise the sums alone
int cluster_pass(pmf_ctx* c, bool assign) {
  PMFCHK(cluster_alloc(c));
  if (!assign && c->algo == PMF_ALGO_KMEANS && !c->cl_have_asg)
    return fail(c, PMF_EINVAL, "Kmeans: update_w needs an assignment (update_h has not run)");
  if (assign) {
    if (!c->cl_mu_valid) {                         // once per uploaded V
      hipLaunchKernelGGL(k_cluster_rowmean, dim3((unsigned)c->mp), dim3(256), 0, c->stream, c->dV, (int64_t)c->np, (int)c->n, c->dClMu);
      HIPCHK(c, hipGetLastError());
      c->cl_mu_valid = true;
    }
    hipLaunchKernelGGL(k_cluster_wnorm, dim3((unsigned)c->KP), dim3(256), 0, c->stream, c->dW, c->dClMu, c->mp, c->KP, c->dClWn);
    HIPCHK(c, hipGetLastError());
  }
  ClusterArgs a{};
  a.V = c->dV; a.W = c->dW; a.H = c->dH; a.mu = c->dClMu; a.asg = c->dClAsg; a.wn = c->dClWn;
  a.num = c->dClNum; a.den = c->dClDen; a.err = c->dClErr;
  a.mp = c->mp; a.np = c->np; a.n = (int)c->n; a.k = c->k; a.npanels = c->np / 64; a.panels_per_wg = c->cl_ppw;
  a.assign = assign ? 1 : 0;
  a.expo = (float)(2.0 / (1.75 - 1.0));          // cmeans.py:73,79
  stat_begin(c, SITE_CLUSTER);
  switch (c->NT) {
    case 1: PMFCHK(cluster_launch_t<1>(c, a)); break;
    case 2: PMFCHK(cluster_launch_t<2>(c, a)); break;
    case 4: PMFCHK(cluster_launch_t<4>(c, a)); break;
    default: PMFCHK(cluster_launch_t<8>(c, a)); break;
  }
  stat_end(c, SITE_CLUSTER);
  hipLaunchKernelGGL(k_cluster_totals, dim3(1), dim3(256), 0, c->stream, c->dClDen, c->dClErr, c->cl_wgs, c->KP, c->dClTot);
  HIPCHK(c, hipGetLastError());
  if (assign) {
    h_replaced(c, false, true);
    if (c->algo == PMF_ALGO_KMEANS) c->cl_have_asg = true;
  }
  c->cl_sums_valid = true;
  c->cl_err_valid = assign && c->algo == PMF_ALGO_KMEANS;   // dClTot[KP] = ||V - W H||^2 of the W, H at hand
  return PMF_OK;
}

int cluster_update_h(pmf_ctx* c) { return cluster_csr(c) ? cluster_csr_update_h(c) : cluster_pass(c, true); }

int cluster_update_w(pmf_ctx* c) {
  if (cluster_csr(c)) return cluster_csr_update_w(c);
  if (!c->cl_sums_valid) PMFCHK(cluster_pass(c, false));
  const int64_t elems = c->mp * c->KP;
  const dim3 grid((unsigned)((elems + 255) / 256));
  if (c->algo == PMF_ALGO_KMEANS)
    hipLaunchKernelGGL(k_cluster_finish<PMF_CL_KMEANS>, grid, dim3(256), 0, c->stream, c->dClNum, c->cl_wgs, elems, c->KP, c->dClTot, c->dW);
  else
    hipLaunchKernelGGL(k_cluster_finish<PMF_CL_CMEANS>, grid, dim3(256), 0, c->stream, c->dClNum, c->cl_wgs, elems, c->KP, c->dClTot, c->dW);
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  c->cl_err_valid = false;
  return PMF_OK;
}

// ||V - W H||: Kmeans right behind its own assignment has it as sum_c min_j d^2, unless that is below 1e-3 of the centred
// ||V - mu||^2 (tight clusters: the expansion has cancelled, the rule of nmf_error / cnmf_error); everything else takes
// the direct residual
int cluster_error(pmf_ctx* c, double* out) {
  if (cluster_csr(c)) return cluster_csr_error(c, out);
  if (!c->cl_err_valid) return frobenius_direct(c, out);
  double t[2] = {0.0, 0.0};                        // sum_c min_j d^2, sum_c ||v_c - mu||^2
  HIPCHK(c, hipMemcpyAsync(t, c->dClTot + c->KP, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!(t[0] > 1e-3 * t[1])) return frobenius_direct(c, out);
  *out = std::sqrt(t[0]);
  return PMF_OK;
}

// pmf_frobenius: the direct residual on dense data, as before; on CSR data the error of the steps
int cluster_frobenius(pmf_ctx* c, double* out) { return cluster_csr(c) ? cluster_csr_error(c, out) : frobenius_direct(c, out); }

}  // namespace
