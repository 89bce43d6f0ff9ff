// pmf_host_nndsvd.h -- NNDSVD initialisation with the top-k eigen solver (kernels: pmf_nndsvd.h, pmf_topk.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// ---- NNDSVD initialisation (pymf/nndsvd.py:79-108; kernels and the closed form: pmf_nndsvd.h) ----
struct DevTemps {                 // scratch of one pmf_nndsvd_init call
  pmf_ctx* c = nullptr;
  std::vector<void*> p;
  ~DevTemps() { for (void* q : p) (void)dfree(c, &q); }
};

template <typename T>
int talloc(pmf_ctx* c, DevTemps& t, T** out, size_t count) {
  PMFCHK(dalloc(c, out, count));
  t.c = c;
  t.p.push_back(*out);
  return PMF_OK;
}

// Ad [np][np] (float64) = V^T V of the dense V, summed over all ranks: 128 (or 64) Gram rows per pass of
// k_colgemm with the column block of V as its "W" operand (fp32 MFMA products, float64 slab sums).
// slab: gchunks * 128 * (np + 128) floats of scratch; rpc rows per chunk.
int gram_vtv(pmf_ctx* c, double* Ad, float* slab, int gchunks, int rpc) {
  const int np = c->np;
  // block row c0 against the columns from c0 on only (the matrix is symmetric: half the products), mirrored at the end
  for (int c0 = 0; c0 < np;) {
    const int wdt = (np - c0 >= 128) ? 128 : 64;
    const int xn = np - c0;
    if (wdt == 128) PMFCHK((launch_colgemm<8, false>(c, c->dV + c0, np, xn, c->dV + c0, np, c->mp, rpc, gchunks, slab)));
    else PMFCHK((launch_colgemm<4, false>(c, c->dV + c0, np, xn, c->dV + c0, np, c->mp, rpc, gchunks, slab)));
    // (one thread per element walking the slabs one load at a time took 0.2 ms per pass at 512 slabs)
    hipLaunchKernelGGL((k_reduce_slabs_block<double>), dim3((unsigned)(((int64_t)wdt * xn / 4 + 63) / 64)), dim3(1024), 0, c->stream, slab,
                       gchunks, wdt, xn + wdt, xn, Ad + (size_t)c0 * np + c0, (int64_t)np, 0);
    HIPCHK(c, hipGetLastError());
    c0 += wdt;
  }
  hipLaunchKernelGGL(k_mirror_upper_f64, dim3((unsigned)(((int64_t)np * np + 255) / 256)), dim3(256), 0, c->stream, Ad, np);
  HIPCHK(c, hipGetLastError());
  return allreduce_sum(c, Ad, (size_t)np * np, true);
}

// ---- top-k eigenpairs of the Gram matrix (pmf_topk.h) ----------------------------------------------
// C[M x N] = A[M x K] B, B stored [K][N] (or [N][K]: transb); M, N, K multiples of 16; float64 MFMA.
int dgemm64(pmf_ctx* c, const double* A, int64_t lda, const double* B, int64_t ldb, int K, double* C, int64_t ldc, int M, int N,
            bool transb) {
  const dim3 grid((unsigned)(N / 16), (unsigned)(M / 16));
  if (transb) hipLaunchKernelGGL((k_dgemm_mfma<true>), grid, dim3(64), 0, c->stream, A, lda, B, ldb, K, C, ldc, (float*)nullptr, (int64_t)0, (const int*)nullptr);
  else hipLaunchKernelGGL((k_dgemm_mfma<false>), grid, dim3(64), 0, c->stream, A, lda, B, ldb, K, C, ldc, (float*)nullptr, (int64_t)0, (const int*)nullptr);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// eigen-decomposition of the nj x nj (nj even) symmetric A (leading dimension ld, as A2 and QT) on the device: evals
// (unsorted), rows of QT
int jacobi_eigh_dev(pmf_ctx* c, double* A, double* A2, double* QT, int ld, int nj, double* evals, int* sweeps_done) {
  const int64_t items = (int64_t)(nj / 2) * (nj / 2) + (int64_t)(nj / 2) * nj;
  int dev = 0, cus = 256;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
  const int64_t max_wgs = nj > 1024 ? cus : 64;      // one 1024-thread workgroup per CU at most (cooperative launch)
  const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min<int64_t>(max_wgs, items / 4096));
  int ld_ = ld, nj_ = nj, sweeps_ = 40;
  void* args[] = {&A, &A2, &QT, &ld_, &nj_, &sweeps_, &evals, &sweeps_done};
  HIPCHK(c, hipLaunchCooperativeKernel(reinterpret_cast<const void*>(&k_jacobi_eigh), dim3(wgs), dim3(1024), args,
                                       (unsigned)jacobi_smem_bytes(nj), c->stream));
  return PMF_OK;
}

// The k largest eigenpairs of G [np][np] (symmetric positive semi-definite, rows / columns >= n zero): rows 0 .. nl-1 of L
// ([round_up(k, 16)][np], zeroed by the caller) and ev[0 .. nl-1], descending as locked; nl <= k.  pmf_topk.h has the method.
int eigh_topk(pmf_ctx* c, DevTemps& tmp, double* G, int n, int np, int k, double* L, double* ev_dev, int* nl_out, int* products_out) {
  const int ld = np;
  const int kp16 = (int)round_up(k, 16);
  const int pblk = std::max(16, std::min(64, k / 2));
  const int s = (int)std::min<int64_t>(round_up(k + pblk, 16), (n / 16) * 16);
  if (s < 16 || s < k) return fail(c, PMF_EINVAL, "eigh_topk: the block does not fit the matrix");
  const int64_t cnt = (int64_t)s * ld;
  double *Ya, *Yb, *Yc, *Z, *D, *GQ, *T1, *S, *S2, *QTs, *Ug, *C1, *dth, *dev_ev, *dsc, *dres;
  int *dperm, *dinfo;
  for (double** q : {&Ya, &Yb, &Yc, &Z, &D, &GQ, &T1}) PMFCHK(talloc(c, tmp, q, (size_t)cnt));
  for (double** q : {&S, &S2, &QTs, &Ug}) PMFCHK(talloc(c, tmp, q, (size_t)s * s));
  PMFCHK(talloc(c, tmp, &C1, (size_t)s * kp16));
  PMFCHK(talloc(c, tmp, &dth, (size_t)kp16));
  PMFCHK(talloc(c, tmp, &dev_ev, (size_t)s));
  PMFCHK(talloc(c, tmp, &dsc, (size_t)s));
  PMFCHK(talloc(c, tmp, &dres, (size_t)s));
  PMFCHK(talloc(c, tmp, &dperm, (size_t)s));
  PMFCHK(talloc(c, tmp, &dinfo, 2));
  std::vector<double> th(s), hev(s), hsc(s), hres(s), thl;
  std::vector<int> perm(s);
  int nl = 0, products = 0;
  uint64_t seed = 0x9e3779b97f4a7c15ull;
  auto blocks = [](int64_t count) { return dim3((unsigned)((count + 255) / 256)); };
  auto fill_random = [&](double* Y, int r0, int r1) -> int {
    hipLaunchKernelGGL(k_topk_fill_random, blocks((int64_t)(r1 - r0) * ld), dim3(256), 0, c->stream, Y, r0, r1, ld, n, seed++);
    HIPCHK(c, hipGetLastError());
    return PMF_OK;
  };
  // D = (Y L^T) diag(theta or 1) L : the locked directions' part of Y (scaled: of A Y)
  auto locked_part = [&](const double* Y, bool scaled) -> int {
    PMFCHK(dgemm64(c, Y, ld, L, ld, np, C1, kp16, s, kp16, true));
    if (scaled) {
      hipLaunchKernelGGL(k_topk_scale_cols, blocks((int64_t)s * kp16), dim3(256), 0, c->stream, C1, s, kp16, kp16, dth);
      HIPCHK(c, hipGetLastError());
    }
    return dgemm64(c, C1, kp16, L, ld, kp16, D, ld, s, np, false);
  };
  // Zout = Y A'  (A' = A with the locked pairs deflated); returns with D = the deflation term when with_d
  auto apply = [&](const double* Y, double* Zout) -> int {
    ++products;
    PMFCHK(dgemm64(c, Y, ld, G, ld, np, Zout, ld, s, np, false));
    if (nl > 0) PMFCHK(locked_part(Y, true));
    return PMF_OK;
  };
  auto eigh_small = [&](double* A) -> int {                     // A (s x s) -> QTs rows, hev (host, unsorted)
    PMFCHK(jacobi_eigh_dev(c, A, S2, QTs, s, s, dev_ev, dinfo));
    HIPCHK(c, hipMemcpyAsync(hev.data(), dev_ev, (size_t)s * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PMF_OK;
  };
  auto ortho = [&](double*& Y) -> int {
    for (int attempt = 0; attempt < 4; ++attempt) {
      if (nl > 0)
        for (int rep = 0; rep < 2; ++rep) {
          PMFCHK(locked_part(Y, false));
          hipLaunchKernelGGL(k_topk_sub, blocks(cnt), dim3(256), 0, c->stream, Y, D, cnt);
          HIPCHK(c, hipGetLastError());
        }
      bool deficient = false;
      for (int rep = 0; rep < 2 && !deficient; ++rep) {
        PMFCHK(dgemm64(c, Y, ld, Y, ld, np, S, s, s, s, true));
        PMFCHK(eigh_small(S));
        double lmax = 0.0;
        for (int j = 0; j < s; ++j) lmax = std::max(lmax, hev[j]);
        if (!(lmax > 0.0) || !std::isfinite(lmax)) return fail(c, PMF_EHIP, "eigh_topk: the block collapsed");
        for (int j = 0; j < s; ++j) {
          if (!(hev[j] > 1e-24 * lmax)) { deficient = true; hsc[j] = 0.0; }
          else hsc[j] = 1.0 / std::sqrt(hev[j]);
        }
        HIPCHK(c, hipMemcpyAsync(dsc, hsc.data(), (size_t)s * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PMFCHK(dgemm64(c, QTs, s, Y, ld, s, T1, ld, s, np, false));
        hipLaunchKernelGGL(k_topk_scale_rows, blocks(cnt), dim3(256), 0, c->stream, T1, s, ld, dsc);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));               // hsc is reused
        std::swap(Y, T1);
        if (deficient)                                            // dependent rows came out as zeros: new random ones, again
          for (int j = 0; j < s; ++j)
            if (hsc[j] == 0.0) PMFCHK(fill_random(Y, j, j + 1));
      }
      if (!deficient) return PMF_OK;
    }
    return fail(c, PMF_EHIP, "eigh_topk: could not orthonormalise the block");
  };
  // Rayleigh-Ritz on the orthonormal rows Y: GQ = Y A', T = Y GQ^T, rows rotated to the Ritz vectors, th descending
  auto rayleigh_ritz = [&](double*& Y) -> int {
    PMFCHK(apply(Y, GQ));
    if (nl > 0) {
      hipLaunchKernelGGL(k_topk_sub, blocks(cnt), dim3(256), 0, c->stream, GQ, D, cnt);
      HIPCHK(c, hipGetLastError());
    }
    PMFCHK(dgemm64(c, Y, ld, GQ, ld, np, S, s, s, s, true));
    PMFCHK(eigh_small(S));
    for (int j = 0; j < s; ++j) perm[j] = j;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return hev[a] > hev[b]; });
    for (int j = 0; j < s; ++j) th[j] = hev[perm[j]];
    HIPCHK(c, hipMemcpyAsync(dperm, perm.data(), (size_t)s * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dev_ev, th.data(), (size_t)s * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_topk_gather_rows, blocks((int64_t)s * s), dim3(256), 0, c->stream, QTs, (int64_t)s, dperm, Ug, (int64_t)s, s, s);
    HIPCHK(c, hipGetLastError());
    PMFCHK(dgemm64(c, Ug, s, Y, ld, s, T1, ld, s, np, false));
    std::swap(Y, T1);
    PMFCHK(dgemm64(c, Ug, s, GQ, ld, s, T1, ld, s, np, false));
    std::swap(GQ, T1);
    hipLaunchKernelGGL(k_topk_resid, dim3((unsigned)s), dim3(256), 0, c->stream, GQ, Y, ld, np, dev_ev, dres);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hres.data(), dres, (size_t)s * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PMF_OK;
  };

  hipLaunchKernelGGL(k_topk_symmetrise, blocks((int64_t)n * n), dim3(256), 0, c->stream, G, ld, n);
  HIPCHK(c, hipGetLastError());
  PMFCHK(fill_random(Ya, 0, s));
  PMFCHK(ortho(Ya));
  PMFCHK(rayleigh_ritz(Ya));
  const double scale = std::max(th[0], 1e-300);
  // A pair is locked when its residual is below 1e-11 of ITS OWN eigenvalue: the error of the vector is residual / gap, and
  // a tolerance relative to lambda_1 cannot be met by the dominant pair itself (its rounding floor is ~1e-12 lambda_1 at
  // n = 4608) while being too loose for the pairs of the bulk (1e-13 lambda_1 = 6e-7 against gaps of 0.05 there).
  double tol = 1e-11, prev_lead = 1e300;
  int stagnant = 0;
  constexpr int kMaxIter = 300, kMaxDeg = 40;
  for (int it = 0; it < kMaxIter && nl < k; ++it) {
    // ---- lock the leading converged pairs, in order ----
    const int need = k - nl;
    if (std::getenv("PMF_TOPK_DEBUG")) fprintf(stderr, "topk it %d: locked %d products %d th[0] %.6e th[need-1] %.6e th[s-1] %.6e res[0]/th %.2e res[need-1]/th %.2e\n", it, nl, products, th[0], th[std::min(need, s) - 1], th[s - 1], hres[0] / std::max(th[0], 1e-300), hres[std::min(need, s) - 1] / std::max(th[std::min(need, s) - 1], 1e-300));
    int nlock = 0;
    while (nlock < std::min(need, s) && (hres[nlock] <= tol * th[nlock] || th[nlock] <= 1e-14 * scale)) ++nlock;
    // the leading pair sits on its rounding floor (its residual no longer halves from one filter to the next; at
    // n = 16 384 the floor of the bulk pairs is 3e-10 of their eigenvalue: the deflated lambda_1 leaves eps lambda_1 behind):
    // take the floor as the tolerance
    const double lead = hres[0] / std::max(th[0], 1e-300);
    if (nlock == 0) {
      stagnant = (lead > 0.5 * prev_lead) ? stagnant + 1 : 0;
      if (stagnant >= 2 || it > kMaxIter - 3) {
        if (lead > 1e-8) return fail(c, PMF_EHIP, "pmf_nndsvd_init: the top-k eigen-solver stalled (residual " + std::to_string(lead) + " of the eigenvalue)");
        tol = std::max(tol, 2.0 * lead);
        stagnant = 0;
        prev_lead = 1e300;
        continue;
      }
    }
    prev_lead = nlock > 0 ? 1e300 : lead;
    if (nlock > 0) stagnant = 0;
    if (nlock > 0) {
      HIPCHK(c, hipMemcpyAsync(L + (size_t)nl * ld, Ya, (size_t)nlock * ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      for (int j = 0; j < nlock; ++j) thl.push_back(th[j]);
      nl += nlock;
      HIPCHK(c, hipMemcpyAsync(dth, thl.data(), (size_t)nl * sizeof(double), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (nl >= k) break;
      // the rest of the block moves up, fresh random rows behind it
      HIPCHK(c, hipMemcpyAsync(T1, Ya + (size_t)nlock * ld, (size_t)(s - nlock) * ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      std::swap(Ya, T1);
      PMFCHK(fill_random(Ya, s - nlock, s));
      PMFCHK(ortho(Ya));
      PMFCHK(rayleigh_ritz(Ya));
      continue;
    }
    // ---- Chebyshev filter: damp [0, cut], degree bounded by the dynamic range inside the block ----
    const double cut = std::max(th[s - 1], 1e-10 * scale), top = std::max(th[0], cut * (1.0 + 1e-12));
    const double e = 0.5 * cut, cc = 0.5 * cut;
    const double x_top = (top - cc) / e, x_k = (std::max(th[std::min(need, s) - 1], cut) - cc) / e;
    int deg = kMaxDeg;
    {
      const double g_top = std::acosh(std::max(x_top, 1.0)), g_k = std::acosh(std::max(x_k, 1.0));
      if (g_top - g_k > 0.0) deg = (int)std::max(2.0, std::min((double)kMaxDeg, std::floor(std::log(1e9) / (g_top - g_k))));
    }
    double sigma = e / (top - cc);
    const double sigma1 = sigma;
    PMFCHK(apply(Ya, Z));
    hipLaunchKernelGGL(k_topk_cheb, blocks(cnt), dim3(256), 0, c->stream, Z, nl > 0 ? D : nullptr, Ya, (const double*)nullptr, Yb, cnt, cc,
                       sigma1 / e, 0.0);
    HIPCHK(c, hipGetLastError());
    for (int d = 2; d <= deg; ++d) {
      const double sigma2 = 1.0 / (2.0 / sigma1 - sigma);
      PMFCHK(apply(Yb, Z));
      hipLaunchKernelGGL(k_topk_cheb, blocks(cnt), dim3(256), 0, c->stream, Z, nl > 0 ? D : nullptr, Yb, Ya, Yc, cnt, cc, 2.0 * sigma2 / e,
                         sigma * sigma2);
      HIPCHK(c, hipGetLastError());
      double* t = Ya; Ya = Yb; Yb = Yc; Yc = t;
      sigma = sigma2;
    }
    std::swap(Ya, Yb);
    PMFCHK(ortho(Ya));
    PMFCHK(rayleigh_ritz(Ya));
  }
  // out of iterations with pairs still unlocked whose Ritz values are NOT negligible: the solver did not converge (the
  // caller falls back to Jacobi where that exists) -- "fewer than num_bases eigenvalues" would be the wrong diagnosis
  if (nl < k && th[0] > 1e-14 * scale)
    return fail(c, PMF_EHIP, "pmf_nndsvd_init: the top-k eigen-solver did not converge (" + std::to_string(nl) + " of " +
                std::to_string(k) + " pairs in " + std::to_string(kMaxIter) + " filter steps)");
  std::vector<double> out(kp16, -1.0);
  for (int j = 0; j < nl && j < kp16; ++j) out[j] = thl[j];
  HIPCHK(c, hipMemcpyAsync(ev_dev, out.data(), (size_t)kp16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *nl_out = nl;
  if (products_out) *products_out = products;
  return PMF_OK;
}

int nndsvd_init(pmf_ctx* c, int32_t* rank_found) {
  if (c->v_csr) return fail(c, PMF_EINVAL, "pmf_nndsvd_init: dense V only");
  if (c->n > PMF_TOPK_MAX_N)
    return fail(c, PMF_EINVAL, "pmf_nndsvd_init: num_samples <= " + std::to_string(PMF_TOPK_MAX_N) +
                " (the Gram matrix is n x n; pass the transposed problem for wide data)");
  if (c->k > c->n) return fail(c, PMF_EINVAL, "pmf_nndsvd_init: num_bases exceeds the number of columns");
  const int n = (int)c->n, np = c->np, KP = c->KP, ld = np;
  // all n eigenpairs by Jacobi (pmf_nndsvd.h: exact and quick up to ~1000 columns, 13 s at 4096), or the k largest by
  // filtered subspace iteration (pmf_topk.h: 0.06 s instead of 1.2 s at 1500 columns, the only form beyond 4096).
  // pmf_set_option("nndsvd_topk", 1 / 0) forces one of them where both apply; a top-k solve that stalls falls back
  // to Jacobi where that exists.
  const bool topk_fits = c->k + 16 <= (n / 16) * 16;
  bool topk = (n > PMF_NNDSVD_MAX_N) || (topk_fits && (c->opt_nndsvd_topk == 1 || (c->opt_nndsvd_topk < 0 && n > 1024)));
  if (topk && !topk_fits) return fail(c, PMF_EINVAL, "pmf_nndsvd_init: num_bases too close to the number of columns for this size");
  int nj = n + (n & 1);
  DevTemps tmp;
  double *Ad = nullptr, *Ad2 = nullptr, *evals = nullptr, *QT = nullptr, *sv = nullptr, *part = nullptr, *norms = nullptr;
  float *slab = nullptr, *B = nullptr, *wscale = nullptr;
  int *order = nullptr, *info = nullptr, *wmode = nullptr;
  const int64_t blocks16 = c->mp / 16;
  int gchunks = (int)std::min<int64_t>(512, blocks16);
  const int rpc = (int)((blocks16 + gchunks - 1) / gchunks) * 16;     // (small chunks on purpose: fp32 sums inside a chunk, float64 across)
  gchunks = (int)((c->mp + rpc - 1) / rpc);
  const int kp16 = (int)round_up(c->k, 16);
  const bool can_jacobi = n <= PMF_NNDSVD_MAX_N;
  PMFCHK(talloc(c, tmp, &Ad, (size_t)np * np));
  PMFCHK(talloc(c, tmp, &evals, (size_t)std::max(np, kp16)));
  PMFCHK(talloc(c, tmp, &slab, (size_t)gchunks * 128 * (np + 128)));
  PMFCHK(talloc(c, tmp, &B, (size_t)KP * np));
  PMFCHK(talloc(c, tmp, &sv, (size_t)KP));
  PMFCHK(talloc(c, tmp, &order, (size_t)KP));
  PMFCHK(talloc(c, tmp, &info, 2));
  PMFCHK(talloc(c, tmp, &wscale, (size_t)KP));
  PMFCHK(talloc(c, tmp, &wmode, (size_t)KP));
  const int nblk = (int)std::min<int64_t>(512, (c->m + 255) / 256);
  const int64_t rows_per_blk = (c->m + nblk - 1) / nblk;
  PMFCHK(talloc(c, tmp, &part, (size_t)nblk * 2 * KP));
  PMFCHK(talloc(c, tmp, &norms, (size_t)2 * KP));

  // 1. A = V^T V over all ranks' rows
  PMFCHK(gram_vtv(c, Ad, slab, gchunks, rpc));
  // 2./3. eigen-decomposition, top-k selection
  if (topk) {
    int nl = 0;
    PMFCHK(talloc(c, tmp, &QT, (size_t)kp16 * np));
    DevTemps work;                                   // the solver's block buffers: freed before the rest of the pipeline
    const int trc = eigh_topk(c, work, Ad, n, np, c->k, QT, evals, &nl, &c->nndsvd_products);
    if (trc == PMF_OK) {
      nj = kp16;                                     // evals[nl ..] = -1: below the reference's 1e-8 cut
    } else if (can_jacobi) {
      topk = false;                                  // (the message of the failed solve is replaced by whatever follows)
    } else {
      return trc;
    }
  }
  if (!topk) {
    PMFCHK(talloc(c, tmp, &QT, (size_t)np * np));
    PMFCHK(talloc(c, tmp, &Ad2, (size_t)np * np));
    PMFCHK(jacobi_eigh_dev(c, Ad, Ad2, QT, ld, nj, evals, info + 1));
  }
  hipLaunchKernelGGL(k_nndsvd_select, dim3(1), dim3(1024), 0, c->stream, evals, QT, ld, nj, n, c->k, KP, np, B, sv,
                     order, info);
  HIPCHK(c, hipGetLastError());
  int hinfo[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(hinfo, info, sizeof(hinfo), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (rank_found) *rank_found = hinfo[0];
  if (hinfo[0] < c->k)
    return fail(c, PMF_EINVAL, "pmf_nndsvd_init: only " + std::to_string(hinfo[0]) + " eigenvalues of data^T data exceed 1e-8 "
                "(svd.py:130-131), fewer than num_bases (the reference raises IndexError at nndsvd.py:94)");
  // 4. U = V (v_i / s_i)  -> dW
  PMFCHK(rowgemm<EPI_STORE>(c, c->dV, np, np, B, np, nullptr, nullptr, c->dW));
  // 5. split norms over all ranks' rows, closed form
  hipLaunchKernelGGL(k_split_norms, dim3((unsigned)nblk, (unsigned)((KP + 255) / 256)), dim3(256), 0, c->stream, c->dW, c->m, KP,
                     rows_per_blk, part);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_split_sum, dim3((unsigned)((2 * KP + 255) / 256)), dim3(256), 0, c->stream, part, nblk, KP, norms);
  HIPCHK(c, hipGetLastError());
  PMFCHK(allreduce_sum(c, norms, (size_t)2 * KP, true));
  hipLaunchKernelGGL(k_nndsvd_finalize, dim3(1), dim3(1024), 0, c->stream, QT, ld, order, sv, norms, n, c->k, KP, np,
                     c->dH, wscale, wmode);
  HIPCHK(c, hipGetLastError());
  const int64_t total = c->mp * KP;
  hipLaunchKernelGGL(k_nndsvd_w, dim3(elem_grid(total)), dim3(256), 0, c->stream, c->dW, total, KP,
                     c->m, wscale, wmode);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  w_replaced(c, /*by_caller=*/false);
  h_replaced(c, false, true);
  return PMF_OK;
}

}  // namespace
