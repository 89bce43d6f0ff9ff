// pmf_host_svd_csr.h -- SVD / PCA on CSR data: the checked upload with its transposed copy, the Gram matrix of the short side from
// stored entries, the projected side, PCA's two steps and the error by the trace identity (kernels: pmf_svd_csr.h, pmf_csr.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
//
// State (pmf_ctx): v_csr on a PCA / SVD context = both CSR images resident (dIndptr ... of V, dTIndptr ... of V^T) and no dense V:
// dV is released by the upload, so every dense-only entry point finds no data.  The eigenpairs are the dense path's buffers
// (dSvdE, dSvdS); the projected side, W and H^T are float64 buffers of their own (dSvdPd, dSvdWd, dSvdHTd): dW, dH and dSvdP are
// not touched.  The Jacobi solver, the 1e-8 cut, the descending order and k_svd_gather are the dense path's own functions
// (eigh_kept, svd_keep in pmf_host_svd.h).
#pragma once

namespace {

bool svd_csr(const pmf_ctx* c) { return c->algo == PMF_ALGO_PCA && c->v_csr; }

// the entry points that have no CSR form on a PCA / SVD context
int svd_csr_refuse(pmf_ctx* c, const char* who) {
  if (!c || !svd_csr(c)) return PMF_OK;
  return fail(c, PMF_EINVAL, std::string(who) + ": not while CSR data is resident on a PCA / SVD context (pmf_svd_decompose, pmf_svd_rank, "
                                                "pmf_svd_get, pmf_update_w, pmf_update_h, pmf_frobenius and the float64 factor transfers "
                                                "work on it; dense data brings the rest back)");
}

// dense data came back to the context: the CSR arrays and the float64 factors go
int svd_csr_left(pmf_ctx* c) {
  if (c->algo != PMF_ALGO_PCA || !c->dIndptr) return PMF_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PMFCHK(dfree(c, &c->dIndptr));
  PMFCHK(dfree(c, &c->dIndices));
  PMFCHK(dfree(c, &c->dVals));
  PMFCHK(dfree(c, &c->dTIndptr));
  PMFCHK(dfree(c, &c->dTIndices));
  PMFCHK(dfree(c, &c->dTVals));
  PMFCHK(dfree(c, &c->dSvdPd));
  PMFCHK(dfree(c, &c->dSvdWd));
  PMFCHK(dfree(c, &c->dSvdHTd));
  PMFCHK(dfree(c, &c->dCslabs));
  std::vector<int64_t>().swap(c->cur_ip);
  c->nnz = 0; c->v_csr = false;
  c->svd_rp = c->svd_wp = 0; c->svd_fact = false;
  c->have_w = c->have_h = false;                       // (the float64 factors were the context's W and H)
  c->path = "svd_gram_f64";
  choose_stat_site(c, false);
  return PMF_OK;
}

// pmf_set_v_csr_f32 on a PCA / SVD context: refused arrays never reach the device and leave the resident data as it was
int svd_csr_set_v(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz) {
  if (c->nranks > 1 || multi_rank(c)) return fail(c, PMF_EINVAL, "pmf_set_v_csr_f32: PCA / SVD on CSR data: one rank only in this build");
  if (std::min<int64_t>(c->mp, c->np) > PMF_GRAM_MAX_NP)
    return fail(c, PMF_EINVAL, "pmf_set_v_csr_f32: PCA / SVD on CSR data: min(rows, cols) > 1024 is not supported by this build");
  const char* why = csr_check(c->m, c->n, indptr, indices, nnz);
  if (!why) why = csr_check_ascending(c->m, indptr, indices);
  if (why) return fail(c, PMF_EINVAL, std::string("pmf_set_v_csr_f32: ") + why);
  CsrPair p;
  csr_transpose_host(c, indptr, indices, vals, nnz, p);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->v_csr) c->have_w = c->have_h = false;        // (the factors of the dense path stay in dW, dH: not the ones read here)
  PMFCHK(dfree(c, &c->dV));                            // a CSR upload replaces dense data
  PMFCHK(csr_upload_pair(c, p, indices, vals, nnz));
  c->cur_ip.assign(indptr, indptr + c->m + 1);
  c->nnz = nnz; c->have_v = true; c->v_csr = true; c->csr_dense = false;
  v_replaced(c);
  c->svd_fact = false;
  c->path = "svd_csr";
  choose_stat_site(c, false);
  return PMF_OK;
}

// Out [lines_p][ldo] float64 = (the image's lines) times B [.][ldb] over the leading `cols` columns (whole 64-column panels)
int svd_csr_proj(pmf_ctx* c, bool transposed, const double* B, int ldb, int cols, double* Out, int ldo, bool timed) {
  const int64_t lines_p = transposed ? (int64_t)c->np : c->mp;
  const int panels = (int)round_up(std::max(cols, 1), 64) / 64;
  if (timed && c->profile && c->stat.site == SITE_SVD) {
    c->stat.name = "k_csr_proj_f64";
    c->stat.flops = c->stat.exec_flops = 2.0 * (double)c->nnz * 64.0 * panels;
    // the entries once per panel, the pointers, the output; the rows of B come from L2
    c->stat.bytes = (12.0 * (double)c->nnz + 8.0 * (double)lines_p + 8.0 * 64.0 * (double)lines_p) * panels;
  }
  const dim3 grid((unsigned)((lines_p + PMF_PROJ_LINES - 1) / PMF_PROJ_LINES), (unsigned)panels);
  if (timed) stat_begin(c, SITE_SVD);
  hipLaunchKernelGGL(k_csr_proj_f64, grid, dim3(256), 0, c->stream, (const int64_t*)(transposed ? c->dTIndptr : c->dIndptr),
                     (const int32_t*)(transposed ? c->dTIndices : c->dIndices), (const float*)(transposed ? c->dTVals : c->dVals), lines_p, B,
                     ldb, Out, ldo);
  if (timed) stat_end(c, SITE_SVD);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// svd.py:160-244 on the resident CSR data.  rows > cols: the eigenpairs of V^T V (the Gram matrix of the columns of the CSR image
// of V) give S and the rows of V, U = data V^T S^-1 on the lines of that image.  Otherwise the eigenpairs of V V^T (the columns of
// the image of V^T) give S and the columns of U, V^T = data^T U S^-1 on the lines of the image of V^T: V is kept transposed,
// [np][rp].  Eigenvalues <= 1e-8 are dropped, the rest sorted descending, the leading svd_triples kept (0: all).
int svd_csr_core(pmf_ctx* c) {
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "SVD: one rank only in this build");
  if (c->svd_valid) return PMF_OK;
  const bool left = c->m > c->n;
  const int q = (int)(left ? c->n : c->m), qp = left ? c->np : (int)c->mp;
  if (qp > PMF_GRAM_MAX_NP) return fail(c, PMF_EINVAL, "SVD on CSR data: min(rows, cols) > 1024 is not supported by this build");
  PMFCHK(svd_alloc(c, false));
  DevTemps tmp;
  double *A = nullptr, *QT = nullptr, *Bd = nullptr;
  PMFCHK(talloc(c, tmp, &A, (size_t)qp * qp));
  if (left) PMFCHK(csr_gram_f64(c, c->dIndptr, c->dIndices, c->dVals, c->nnz, c->m, qp, A));
  else PMFCHK(csr_gram_f64(c, c->dTIndptr, c->dTIndices, c->dTVals, c->nnz, c->n, qp, A));
  std::vector<double> ev;
  std::vector<int> ord;
  PMFCHK(eigh_kept(c, A, q, qp, tmp, ev, ord, &QT));
  if (c->svd_triples > 0 && (int)ord.size() > c->svd_triples) ord.resize((size_t)c->svd_triples);
  const int r = (int)ord.size();
  PMFCHK(svd_keep(c, ev, ord, QT, q, qp, tmp, nullptr));
  const int rp = (int)round_up(std::max(r, 1), 64);
  const int64_t long_p = left ? c->mp : (int64_t)c->np;
  if (rp != c->svd_rp || !c->dSvdPd) {
    c->svd_rp = 0;
    PMFCHK(dgrow(c, &c->dSvdPd, (size_t)long_p * rp));
    c->svd_rp = rp;
  }
  PMFCHK(talloc(c, tmp, &Bd, (size_t)qp * rp));
  hipLaunchKernelGGL(k_svd_csr_b, dim3((unsigned)(((int64_t)qp * rp + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->dSvdE, qp, q, qp, r,
                     rp, (const double*)c->dSvdS, 0, Bd);
  HIPCHK(c, hipGetLastError());
  PMFCHK(svd_csr_proj(c, !left, Bd, rp, rp, c->dSvdPd, rp, true));
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  c->svd_rank = r; c->svd_left = left; c->svd_valid = true;
  return PMF_OK;
}

// pmf_svd_decompose: the factors of pmf_frobenius are W = U and H = S V of the decomposition, read where they lie (svd_csr_error)
int svd_csr_decompose(pmf_ctx* c) {
  PMFCHK(svd_csr_core(c));
  c->have_w = c->have_h = true;
  c->svd_fact = true;
  return PMF_OK;
}

// W [mp][wp] and H^T [np][wp] at width wp: another width drops both factors
int svd_csr_width(pmf_ctx* c, int wp) {
  if (wp == c->svd_wp && c->dSvdWd && c->dSvdHTd) return PMF_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->svd_wp = 0;
  c->have_w = c->have_h = false;
  PMFCHK(dgrow(c, &c->dSvdWd, (size_t)c->mp * wp));
  PMFCHK(dgrow(c, &c->dSvdHTd, (size_t)c->np * wp));
  c->svd_wp = wp;
  return PMF_OK;
}

// PCA.update_w (pca.py:93-108): W = the leading num_bases columns of U (all of them when num_bases == 0), float64
int svd_csr_update_w(pmf_ctx* c) {
  PMFCHK(svd_csr_core(c));
  const int r = c->svd_rank, kb = c->pca_bases > 0 ? std::min(c->pca_bases, r) : r;
  const int wp = (int)round_up(std::max(kb, 1), 64);
  PMFCHK(svd_csr_width(c, wp));
  if (c->svd_left) {
    const int64_t total = c->mp * wp;
    hipLaunchKernelGGL(k_svd_csr_cols, dim3(elem_grid(total)), dim3(256), 0, c->stream, (const double*)c->dSvdPd, c->svd_rp, c->m, total, kb, wp,
                       c->dSvdWd);
  } else {
    hipLaunchKernelGGL(k_svd_csr_b, dim3((unsigned)((c->mp * wp + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->dSvdE, (int)c->mp, (int)c->m,
                       (int)c->mp, kb, wp, (const double*)c->dSvdS, 2, c->dSvdWd);
  }
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  c->svd_fact = false;
  return PMF_OK;
}

// PCA.update_h (pca.py:90-91): H = W^T data, as H^T = data^T W on the lines of the image of V^T
int svd_csr_update_h(pmf_ctx* c) {
  if (c->svd_fact || !c->dSvdWd) return fail(c, PMF_EINVAL, "pmf_update_h on CSR data: no W (pmf_update_w or pmf_set_w_f64 first)");
  PMFCHK(svd_csr_proj(c, true, c->dSvdWd, c->svd_wp, c->svd_wp, c->dSvdHTd, c->svd_wp, true));
  h_replaced(c, false, true);
  return PMF_OK;
}

// G [wp][wp] = X^T Y of X, Y [rows_p][ld] float64 (rows_p a multiple of 64, wp a multiple of 64, wp <= ld)
int svd_csr_tsgram(pmf_ctx* c, const double* X, const double* Y, int ld, int64_t rows_p, int wp, double* G, DevTemps& tmp) {
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(rows_p / 2048, std::max<int64_t>(1, (int64_t)(1 << 22) / ((int64_t)wp * wp))));
  const int64_t chunk_len = round_up((rows_p + want - 1) / want, PMF_TSGRAM_ROWS);
  const int nchunks = (int)((rows_p + chunk_len - 1) / chunk_len);
  double* part = nullptr;
  PMFCHK(talloc(c, tmp, &part, (size_t)nchunks * wp * wp));
  hipLaunchKernelGGL(k_tsgram_f64, dim3((unsigned)(wp / 16), (unsigned)(wp / 16), (unsigned)nchunks), dim3(256), 0, c->stream, X, Y, ld, rows_p,
                     chunk_len, wp, part);
  HIPCHK(c, hipGetLastError());
  const int64_t elems = (int64_t)wp * wp;
  hipLaunchKernelGGL(k_tsgram_reduce_f64, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, c->stream, (const double*)part, nchunks, elems, G);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// <x, y> over n float64 elements: the blocks' sums added in block order on the host.  Synchronises.
int svd_csr_dot(pmf_ctx* c, const double* x, const double* y, int64_t n, double* out, DevTemps& tmp) {
  const int64_t per_block = round_up(std::max<int64_t>(1, (n + PMF_DOT_BLOCKS - 1) / PMF_DOT_BLOCKS), 256);
  const int blocks = (int)((n + per_block - 1) / per_block);
  double* part = nullptr;
  PMFCHK(talloc(c, tmp, &part, (size_t)blocks));
  hipLaunchKernelGGL(k_dot_f64, dim3((unsigned)blocks), dim3(256), 0, c->stream, x, y, n, per_block, part);
  HIPCHK(c, hipGetLastError());
  std::vector<double> h((size_t)blocks);
  HIPCHK(c, hipMemcpyAsync(h.data(), part, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double s = 0.0;
  for (double v : h) s += v;
  *out = s;
  return PMF_OK;
}

// ||data - W H||^2 = ||data||^2 - 2 <W^T data, H> + <W^T W, H H^T>, float64, every sum in a fixed order, clamped at 0 before the
// root.  W [mp][ld], H^T [np][ld], wp live columns (whole panels).  No pass over a dense image and no n x m temporary.
int svd_csr_err(pmf_ctx* c, const double* Wd, const double* HTd, int ld, int wp, double* out) {
  PMFCHK(cur_csr_vnorm2(c, nullptr));
  DevTemps tmp;
  double *X = nullptr, *GW = nullptr, *GH = nullptr;
  PMFCHK(talloc(c, tmp, &X, (size_t)c->np * ld));
  PMFCHK(talloc(c, tmp, &GW, (size_t)wp * wp));
  PMFCHK(talloc(c, tmp, &GH, (size_t)wp * wp));
  PMFCHK(svd_csr_proj(c, true, Wd, ld, wp, X, ld, false));                    // (W^T data)^T; the columns beyond wp stay at the zero of talloc
  double cross = 0.0, quad = 0.0;
  PMFCHK(svd_csr_dot(c, X, HTd, (int64_t)c->np * ld, &cross, tmp));           // (whole buffers: pad lines and pad columns are zero)
  PMFCHK(svd_csr_tsgram(c, Wd, Wd, ld, c->mp, wp, GW, tmp));
  PMFCHK(svd_csr_tsgram(c, HTd, HTd, ld, (int64_t)c->np, wp, GH, tmp));
  PMFCHK(svd_csr_dot(c, GW, GH, (int64_t)wp * wp, &quad, tmp));
  const double f2 = c->cur_vnorm2 - 2.0 * cross + quad;
  *out = std::sqrt(f2 > 0.0 ? f2 : 0.0);
  return PMF_OK;
}

// pmf_frobenius / the error behind PCA's iteration.  Behind pmf_svd_decompose: W = U, H = S V, with S on the eigenvector side
// (W H = (U S) V), so the projected side is read as it lies and the scaled eigenvectors are a [short side][rp] temporary.
int svd_csr_error(pmf_ctx* c, double* out) {
  if (c->svd_fact && c->svd_valid) {
    const int rp = c->svd_rp, qp = c->svd_left ? c->np : (int)c->mp, q = (int)(c->svd_left ? c->n : c->m);
    DevTemps tmp;
    double* T = nullptr;
    PMFCHK(talloc(c, tmp, &T, (size_t)qp * rp));
    hipLaunchKernelGGL(k_svd_csr_b, dim3((unsigned)(((int64_t)qp * rp + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->dSvdE, qp, q, qp,
                       c->svd_rank, rp, (const double*)c->dSvdS, 1, T);
    HIPCHK(c, hipGetLastError());
    return c->svd_left ? svd_csr_err(c, c->dSvdPd, T, rp, rp, out) : svd_csr_err(c, T, c->dSvdPd, rp, rp, out);
  }
  if (c->svd_fact || !c->dSvdWd || !c->dSvdHTd) return fail(c, PMF_EINVAL, "pmf_frobenius on CSR data: no factors of the current data");
  return svd_csr_err(c, c->dSvdWd, c->dSvdHTd, c->svd_wp, c->svd_wp, out);
}

// U (rows x r), S (r) and V (r x cols) of the last decomposition as float64, row-major; any of them may be null
int svd_csr_get(pmf_ctx* c, double* U, double* S, double* V) {
  if (!c->svd_valid) return fail(c, PMF_EINVAL, "pmf_svd_get: no decomposition of the current data (pmf_svd_decompose / pmf_update_w first)");
  const int r = c->svd_rank, rp = c->svd_rp;
  const int64_t m = c->m, n = c->n;
  const int qp = c->svd_left ? c->np : (int)c->mp;
  if (r == 0) return PMF_OK;
  if (S) HIPCHK(c, hipMemcpyAsync(S, c->dSvdS, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  std::vector<double> E, P;
  if ((c->svd_left && V) || (!c->svd_left && U)) {
    E.resize((size_t)r * qp);
    HIPCHK(c, hipMemcpyAsync(E.data(), c->dSvdE, E.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  if ((c->svd_left && U) || (!c->svd_left && V)) {
    P.resize((size_t)(c->svd_left ? m : n) * rp);
    HIPCHK(c, hipMemcpyAsync(P.data(), c->dSvdPd, P.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->svd_left) {
    if (V) for (int i = 0; i < r; ++i) std::memcpy(V + (size_t)i * n, E.data() + (size_t)i * qp, (size_t)n * sizeof(double));
    if (U) for (int64_t row = 0; row < m; ++row) std::memcpy(U + (size_t)row * r, P.data() + (size_t)row * rp, (size_t)r * sizeof(double));
  } else {
    if (U) for (int64_t row = 0; row < m; ++row) for (int i = 0; i < r; ++i) U[(size_t)row * r + i] = E[(size_t)i * qp + row];
    if (V) for (int i = 0; i < r; ++i) for (int64_t col = 0; col < n; ++col) V[(size_t)i * n + col] = P[(size_t)col * rp + i];
  }
  return PMF_OK;
}

// ---- the factor transfers while CSR data is resident: float64 on the device, the caller's [m][k] and [k][n] layouts -------------
int svd_csr_set_w(pmf_ctx* c, const void* W, bool f64) {
  PMFCHK(svd_csr_width(c, (int)round_up(c->k, 64)));
  const int wp = c->svd_wp, k = c->k;
  std::vector<double> h((size_t)c->m * wp, 0.0);
  for (int64_t r = 0; r < c->m; ++r)
    for (int i = 0; i < k; ++i)
      h[(size_t)r * wp + i] = f64 ? static_cast<const double*>(W)[(size_t)r * k + i] : (double)static_cast<const float*>(W)[(size_t)r * k + i];
  HIPCHK(c, hipMemcpyAsync(c->dSvdWd, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  w_replaced(c, true);
  c->svd_fact = false;
  return PMF_OK;
}

int svd_csr_set_h(pmf_ctx* c, const void* H, bool f64) {
  PMFCHK(svd_csr_width(c, (int)round_up(c->k, 64)));
  const int wp = c->svd_wp, k = c->k;
  const int64_t n = c->n;
  std::vector<double> h((size_t)n * wp, 0.0);
  for (int i = 0; i < k; ++i)
    for (int64_t col = 0; col < n; ++col)
      h[(size_t)col * wp + i] = f64 ? static_cast<const double*>(H)[(size_t)i * n + col] : (double)static_cast<const float*>(H)[(size_t)i * n + col];
  HIPCHK(c, hipMemcpyAsync(c->dSvdHTd, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  h_replaced(c, false, true);
  c->svd_fact = false;
  return PMF_OK;
}

template <typename T>
int svd_csr_get_w(pmf_ctx* c, T* W) {
  if (c->svd_fact || !c->dSvdWd) return fail(c, PMF_EINVAL, "W on CSR data: behind pmf_svd_decompose the factors are read through pmf_svd_get");
  const int wp = c->svd_wp, k = c->k;
  std::vector<double> h((size_t)c->m * wp);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->dSvdWd, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int64_t r = 0; r < c->m; ++r)
    for (int i = 0; i < k; ++i) W[(size_t)r * k + i] = i < wp ? (T)h[(size_t)r * wp + i] : (T)0;
  return PMF_OK;
}

template <typename T>
int svd_csr_get_h(pmf_ctx* c, T* H) {
  if (c->svd_fact || !c->dSvdHTd) return fail(c, PMF_EINVAL, "H on CSR data: behind pmf_svd_decompose the factors are read through pmf_svd_get");
  const int wp = c->svd_wp, k = c->k;
  const int64_t n = c->n;
  std::vector<double> h((size_t)n * wp);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->dSvdHTd, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < k; ++i)
    for (int64_t col = 0; col < n; ++col) H[(size_t)i * n + col] = i < wp ? (T)h[(size_t)col * wp + i] : (T)0;
  return PMF_OK;
}

}  // namespace
