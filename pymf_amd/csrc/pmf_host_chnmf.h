// pmf_host_chnmf.h -- CHNMF: the projection, the hull passes of all pairs enqueued back to back, the three routes of a pair
// (filter with 32 directions -> chain; rerun with 128 directions; chain on the host), the union (kernels: pmf_chnmf.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

constexpr int PMF_CH_MAX_PAIRS = PMF_CH_MAX_SEL * (PMF_CH_MAX_SEL - 1) / 2;

int chnmf_cap(const pmf_ctx* c) { return c->ch_cap > 0 ? c->ch_cap : PMF_CH_CAP; }

int chnmf_alloc(pmf_ctx* c) {
  if (c->dChProj) return PMF_OK;
  PMFCHK(dalloc(c, &c->dChR, (size_t)PMF_CH_MAX_SEL * c->mp));
  PMFCHK(dalloc(c, &c->dChPscore, (size_t)PMF_CL_MAX_WGS * PMF_CH_D1));
  PMFCHK(dalloc(c, &c->dChPidx, (size_t)PMF_CL_MAX_WGS * PMF_CH_D1));
  PMFCHK(dalloc(c, &c->dChPmax, (size_t)PMF_CL_MAX_WGS));
  PMFCHK(dalloc(c, &c->dChEdges, (size_t)PMF_CH_D1 * PMF_CH_EDGE));
  PMFCHK(dalloc(c, &c->dChCounts, (size_t)PMF_CL_MAX_WGS));
  PMFCHK(dalloc(c, &c->dChSurv, (size_t)PMF_CH_CAP));
  PMFCHK(dalloc(c, &c->dChNsurv, (size_t)PMF_CH_MAX_PAIRS + 1));      // [PMF_CH_MAX_PAIRS]: the size of the union
  PMFCHK(dalloc(c, &c->dChKeep, (size_t)c->np));
  PMFCHK(dalloc(c, &c->dChMask, (size_t)c->np));
  PMFCHK(dalloc(c, &c->dChIdx, (size_t)c->np));
  PMFCHK(dalloc(c, &c->dChProj, (size_t)PMF_CH_MAX_SEL * c->np));
  return PMF_OK;
}

// proj = R V (chnmf.py:180-181), R [base_sel][m] float64 from the host
int chnmf_project(pmf_ctx* c, const double* R, int base_sel) {
  std::vector<double> Rp((size_t)PMF_CH_MAX_SEL * c->mp, 0.0);
  for (int i = 0; i < base_sel; ++i) std::copy_n(R + (size_t)i * c->m, (size_t)c->m, Rp.begin() + (size_t)i * c->mp);
  HIPCHK(c, hipMemcpyAsync(c->dChR, Rp.data(), Rp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (Rp leaves with this frame)
  hipLaunchKernelGGL(k_chnmf_proj, dim3((unsigned)((c->np + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->dChR, (const float*)c->dV, c->mp,
                     c->np, (int)round_up(c->m, 4), c->dChProj);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// the two stages of pair `pair` = rows (i, j) of proj with D directions; the survivor count stays in dChNsurv[pair]
int chnmf_pair(pmf_ctx* c, int pair, int i, int j, int D, int ppw, int wgs) {
  const int cap = chnmf_cap(c);
  int P = 1;
  while (P < cap) P <<= 1;
  HullArgs a{};
  a.px = c->dChProj + (size_t)i * c->np; a.py = c->dChProj + (size_t)j * c->np;
  a.n = (int)c->n; a.npanels = c->np / 64; a.panels_per_wg = ppw; a.wgs = wgs; a.D = D;
  a.pscore = c->dChPscore; a.pidx = c->dChPidx; a.pmax = c->dChPmax; a.edges = c->dChEdges; a.keep = c->dChKeep; a.counts = c->dChCounts;
  hipLaunchKernelGGL(k_hull_extremes, dim3((unsigned)wgs, (unsigned)(D / PMF_CH_DCHUNK)), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_hull_polygon, dim3(1), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_hull_filter, dim3((unsigned)wgs), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_hull_compact, dim3((unsigned)wgs), dim3(256), 0, c->stream, (const unsigned char*)c->dChKeep, (const int*)c->dChCounts, wgs,
                     a.npanels, ppw, cap, c->dChSurv, c->dChNsurv + pair);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_hull_chain, dim3(1), dim3(1024), hull_chain_smem(P), c->stream, a.px, a.py, (const int*)c->dChSurv,
                     (const int*)(c->dChNsurv + pair), cap, P, (int)c->n, c->dChMask);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// the third route: the pair's rows on the host, sorted by (x, y, index), the same chain; its vertices are marked in the mask
int chnmf_pair_host(pmf_ctx* c, int i, int j) {
  const size_t n = (size_t)c->n;
  std::vector<double> x(n), y(n);
  HIPCHK(c, hipMemcpyAsync(x.data(), c->dChProj + (size_t)i * c->np, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(y.data(), c->dChProj + (size_t)j * c->np, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<int> ord(n);
  for (size_t q = 0; q < n; ++q) ord[q] = (int)q;
  std::sort(ord.begin(), ord.end(), [&](int p, int q) { return x[p] < x[q] || (x[p] == x[q] && (y[p] < y[q] || (y[p] == y[q] && p < q))); });
  std::vector<int> verts;
  for (int side = 0; side < 2; ++side) {
    std::vector<int> st;
    for (size_t q = 0; q < n; ++q) {
      const size_t pos = side == 0 ? q : n - 1 - q;
      const int p = ord[pos];
      if (pos > 0 && x[p] == x[ord[pos - 1]] && y[p] == y[ord[pos - 1]]) continue;
      while (st.size() >= 2) {
        const int b = st[st.size() - 1], o = st[st.size() - 2];
        const double cr = (x[b] - x[o]) * (y[p] - y[o]) - (y[b] - y[o]) * (x[p] - x[o]);
        if (cr <= 0.0) st.pop_back(); else break;
      }
      st.push_back(p);
    }
    verts.insert(verts.end(), st.begin(), st.end());
  }
  DevTemps tmp;
  int* dv = nullptr;
  PMFCHK(talloc(c, tmp, &dv, verts.size()));
  HIPCHK(c, hipMemcpyAsync(dv, verts.data(), verts.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_hull_scatter, dim3((unsigned)((verts.size() + 255) / 256)), dim3(256), 0, c->stream, (const int*)dv, (int)verts.size(), (int)c->n,
                     c->dChMask);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));               // the temporaries are released on return
  return PMF_OK;
}

// pmf_chnmf_hull: _hull_idx of chnmf.py:154-183 for the projection matrix R
int chnmf_hull(pmf_ctx* c, const double* R, int base_sel, int32_t* idx_out, int64_t cap_out, int64_t* count_out) {
  PMFCHK(chnmf_alloc(c));
  {
    static bool attr_done_dev[PMF_MAX_DEVICES] = {};        // the attribute is per device
    bool& attr_done = attr_done_dev[pmf_current_device()];
    if (!attr_done) {
      HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hull_chain), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)hull_chain_smem(PMF_CH_CAP)));
      attr_done = true;
    }
  }
  PMFCHK(chnmf_project(c, R, base_sel));
  HIPCHK(c, hipMemsetAsync(c->dChMask, 0, (size_t)c->np, c->stream));
  HIPCHK(c, hipMemsetAsync(c->dChNsurv, 0, ((size_t)PMF_CH_MAX_PAIRS + 1) * sizeof(int), c->stream));
  int ppw = 0, wgs = 0;
  panel_partition(c->np / 64, c->ch_max_wgs > 0 ? c->ch_max_wgs : PMF_CL_MAX_WGS, &ppw, &wgs);
  std::vector<std::pair<int, int>> pairs;                   // itertools.combinations(range(base_sel), 2)
  for (int i = 0; i < base_sel; ++i)
    for (int j = i + 1; j < base_sel; ++j) pairs.emplace_back(i, j);
  const int cap = chnmf_cap(c);
  std::vector<int> todo(pairs.size()), nsurv(pairs.size());
  for (size_t p = 0; p < pairs.size(); ++p) todo[p] = (int)p;
  c->ch_routes[0] = (int)pairs.size(); c->ch_routes[1] = c->ch_routes[2] = 0;
  for (int route = 0; route < 2 && !todo.empty(); ++route) {      // all pairs of a route back to back, then one read of the counts
    for (int p : todo) PMFCHK(chnmf_pair(c, p, pairs[p].first, pairs[p].second, route == 0 ? PMF_CH_D0 : PMF_CH_D1, ppw, wgs));
    HIPCHK(c, hipMemcpyAsync(nsurv.data(), c->dChNsurv, pairs.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> over;
    for (int p : todo)
      if (nsurv[p] > cap) over.push_back(p);
    todo.swap(over);
    c->ch_routes[route] -= (int)todo.size();
    c->ch_routes[route + 1] = (int)todo.size();
  }
  for (int p : todo) PMFCHK(chnmf_pair_host(c, pairs[p].first, pairs[p].second));
  // the union of all pairs' vertices, ascending (np.unique, chnmf.py:168)
  hipLaunchKernelGGL(k_hull_count, dim3((unsigned)wgs), dim3(256), 0, c->stream, (const unsigned char*)c->dChMask, c->np / 64, ppw, c->dChCounts);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_hull_compact, dim3((unsigned)wgs), dim3(256), 0, c->stream, (const unsigned char*)c->dChMask, (const int*)c->dChCounts, wgs, c->np / 64,
                     ppw, c->np, c->dChIdx, c->dChNsurv + PMF_CH_MAX_PAIRS);
  HIPCHK(c, hipGetLastError());
  int total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, c->dChNsurv + PMF_CH_MAX_PAIRS, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *count_out = total;
  if (total > cap_out) return fail(c, PMF_EINVAL, "pmf_chnmf_hull: " + std::to_string(total) + " hull points, idx_out holds " + std::to_string(cap_out));
  if (total > 0) {
    HIPCHK(c, hipMemcpyAsync(idx_out, c->dChIdx, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return PMF_OK;
}

}  // namespace
