// pmf_host_svd.h -- SVD / PCA: svd_dense (svd.py:110-158 for dense data) and the factors PCA takes from it (kernels: pmf_svd.h, pmf_nndsvd.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// chunks of the inner dimension (a multiple of 64) for `ntiles` tiles: tiles x chunks near PMF_SVD_TARGET_WGS, a chunk
// no shorter than PMF_SVD_MIN_CHUNK and a multiple of 64 (64 x 1 048 576: one tile, 512 chunks of 2 048 columns)
void svd_chunks(int inner, int ntiles, int* nchunks, int* chunk_len) {
  const int nch = std::max(1, std::min(PMF_SVD_TARGET_WGS / ntiles, inner / PMF_SVD_MIN_CHUNK));
  *chunk_len = (int)round_up((inner + nch - 1) / nch, 64);
  *nchunks = (inner + *chunk_len - 1) / *chunk_len;
}

// O [.][ldo] float64 = A B^T (A [TA * 64][inner], B [TB * 64][inner]) or A^T B (trans: A [inner][TA * 64], B [inner][TB * 64]) of the
// float32 A, B, zero padded; inner is a multiple of 64.  sym (A == B, TA == TB): the tiles of the upper block triangle only.  The
// product launch is timed as the profiled site `site`.
int prod_f64(pmf_ctx* c, bool trans, bool sym, const float* A, int64_t lda, int TA, const float* B, int64_t ldb, int TB, int inner,
             double* O, int64_t ldo, int site, DevTemps& tmp) {
  const int ntiles = sym ? TB * (TB + 1) / 2 : TA * TB;
  int nch = 1, cl = inner;
  svd_chunks(inner, ntiles, &nch, &cl);
  double* slab = nullptr;
  PMFCHK(talloc(c, tmp, &slab, (size_t)nch * ntiles * PMF_SVD_TILE * PMF_SVD_TILE));
  const auto prod = trans ? (sym ? k_prod_f64<true, true> : k_prod_f64<true, false>) : (sym ? k_prod_f64<false, true> : k_prod_f64<false, false>);
  stat_begin(c, site);
  hipLaunchKernelGGL(prod, dim3((unsigned)ntiles, (unsigned)nch), dim3(256), 0, c->stream, A, lda, B, ldb, inner, cl, TB, slab);
  stat_end(c, site);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(sym ? k_prod_reduce_f64<true> : k_prod_reduce_f64<false>, dim3((unsigned)ntiles * 64u), dim3(1024), 0, c->stream,
                     (const double*)slab, nch, ntiles, TB, O, ldo);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// A [qp][qp] float64 = X X^T (X [qp][inner]) or X^T X (trans: X [inner][qp]) of the float32 X with leading dimension ldx, zero
// padded; qp and inner are multiples of 64
int gram_f64(pmf_ctx* c, const float* X, int64_t ldx, int qp, int inner, bool trans, double* A, DevTemps& tmp) {
  const int T = qp / PMF_SVD_TILE;
  PMFCHK(prod_f64(c, trans, true, X, ldx, T, X, ldx, T, inner, A, (int64_t)qp, SITE_SVD, tmp));
  hipLaunchKernelGGL(k_mirror_upper_f64, dim3((unsigned)(((int64_t)qp * qp + 255) / 256)), dim3(256), 0, c->stream, A, qp);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// The eigenpairs of the float64 q x q matrix A [qp][qp] (overwritten): float64 Jacobi.  ev = the q + (q & 1) eigenvalues (host), ord =
// the indices of those > 1e-8 (svd.py:116-117,141-142) in descending order, QT [.][qp] = the eigenvectors by rows (device, in tmp).
// Synchronises.  The one place of the cut and the order: the dense and the CSR path both come through here.
int eigh_kept(pmf_ctx* c, double* A, int q, int qp, DevTemps& tmp, std::vector<double>& ev, std::vector<int>& ord, double** QT) {
  const int nj = q + (q & 1);
  double *A2 = nullptr, *evals = nullptr;
  int* info = nullptr;
  PMFCHK(talloc(c, tmp, &A2, (size_t)qp * qp));
  PMFCHK(talloc(c, tmp, QT, (size_t)qp * qp));
  PMFCHK(talloc(c, tmp, &evals, (size_t)qp));
  PMFCHK(talloc(c, tmp, &info, 2));
  PMFCHK(jacobi_eigh_dev(c, A, A2, *QT, qp, nj, evals, info));
  ev.resize((size_t)nj);
  HIPCHK(c, hipMemcpyAsync(ev.data(), evals, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ord.clear();
  for (int j = 0; j < nj; ++j)
    if (ev[(size_t)j] > 1e-8) ord.push_back(j);
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return ev[(size_t)a] > ev[(size_t)b]; });
  return PMF_OK;
}

// The singular values of the kept eigenpairs onto the device (dSvdS), and the kept eigenvectors in that order into dSvdE (and, scaled
// by 1 / s, into the float32 B when given): r = ord.size() <= KP
int svd_keep(pmf_ctx* c, const std::vector<double>& ev, std::vector<int>& ord, const double* QT, int q, int qp, DevTemps& tmp, float* B) {
  const int r = (int)ord.size(), KP = c->KP;
  if (r > KP) return fail(c, PMF_EINVAL, "SVD: the rank exceeds the context's base count");
  int* order = nullptr;
  PMFCHK(talloc(c, tmp, &order, (size_t)KP));
  std::vector<double> sv((size_t)KP, 0.0);
  for (int i = 0; i < r; ++i) sv[(size_t)i] = std::sqrt(ev[(size_t)ord[(size_t)i]]);
  ord.resize((size_t)KP, 0);
  HIPCHK(c, hipMemcpyAsync(order, ord.data(), (size_t)KP * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->dSvdS, sv.data(), (size_t)KP * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_svd_gather, dim3((unsigned)(((int64_t)KP * qp + 255) / 256)), dim3(256), 0, c->stream, QT, qp, q, r, KP,
                     (const int*)order, (const double*)c->dSvdS, c->dSvdE, B);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));           // (the host vectors may leave scope)
  return PMF_OK;
}

// The eigenpairs of the q x q Gram matrix of the float32 G (gram_f64's operand), scaled to diag(d) . diag(d) when d (q values on
// the device) is given: float64 Gram matrix, float64 Jacobi.  ev = the q + (q & 1) eigenvalues (host), ord = the indices of those
// > 1e-8 (svd.py:116-117,141-142) in descending order, QT [.][qp] = the eigenvectors by rows (device, in tmp).  Synchronises.
int gram_eigh(pmf_ctx* c, const float* G, int64_t ldg, int q, int qp, int inner, bool trans, const double* d, DevTemps& tmp,
              std::vector<double>& ev, std::vector<int>& ord, double** QT) {
  double* A = nullptr;
  PMFCHK(talloc(c, tmp, &A, (size_t)qp * qp));
  PMFCHK(gram_f64(c, G, ldg, qp, inner, trans, A, tmp));
  if (d) hipLaunchKernelGGL(k_cur_scale_sym, dim3((unsigned)((q * q + 255) / 256)), dim3(256), 0, c->stream, A, qp, q, d);
  HIPCHK(c, hipGetLastError());
  return eigh_kept(c, A, q, qp, tmp, ev, ord, QT);
}

// SVD / PCA on CSR data: pmf_host_svd_csr.h (further down the include order)
bool svd_csr(const pmf_ctx* c);
int svd_csr_decompose(pmf_ctx* c);
int svd_csr_update_w(pmf_ctx* c);
int svd_csr_update_h(pmf_ctx* c);
int svd_csr_error(pmf_ctx* c, double* out);
int svd_csr_get(pmf_ctx* c, double* U, double* S, double* V);

// (the float32 projected side is the dense path's alone: a decomposition of CSR data allocates the other two)
int svd_alloc(pmf_ctx* c, bool with_p = true) {
  const bool left = c->m > c->n;
  if (!c->dSvdE) PMFCHK(dalloc(c, &c->dSvdE, (size_t)c->KP * (left ? c->np : c->mp)));
  if (!c->dSvdS) PMFCHK(dalloc(c, &c->dSvdS, (size_t)c->KP));
  if (with_p && !c->dSvdP) PMFCHK(dalloc(c, &c->dSvdP, left ? (size_t)c->mp * c->KP : (size_t)c->KP * c->np));
  return PMF_OK;
}

// svd.py:110-158 on the resident V.  rows > cols (_left_svd): eigenpairs of V^T V give S and the rows of V (float64, dSvdE),
// U = data V^T S^-1 on k_rowgemm (float32, dSvdP [mp][KP]).  Otherwise (_right_svd): eigenpairs of V V^T give S and the columns
// of U (float64, rows of dSvdE), V = S^-1 U^T data as the W^T V product of W = U S^-1 (float32, dSvdP [KP][np]); dW is left
// holding U S^-1.  Eigenvalues <= 1e-8 are dropped (svd.py:116-117,141-142), the rest sorted descending; svd_rank = how many.
int svd_dense(pmf_ctx* c) {
  if (c->v_csr || !c->dV) return fail(c, PMF_EINVAL, "SVD: dense resident data only");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "SVD: one rank only in this build");
  if (c->svd_valid) return PMF_OK;
  const bool left = c->m > c->n;
  const int q = (int)(left ? c->n : c->m), qp = left ? c->np : (int)c->mp, KP = c->KP;
  PMFCHK(svd_alloc(c));
  DevTemps tmp;
  double* QT = nullptr;
  float* B = nullptr;
  if (left) PMFCHK(talloc(c, tmp, &B, (size_t)KP * qp));
  std::vector<double> ev;
  std::vector<int> ord;
  PMFCHK(gram_eigh(c, c->dV, (int64_t)c->np, q, qp, left ? (int)c->mp : c->np, left, nullptr, tmp, ev, ord, &QT));
  const int r = (int)ord.size();
  PMFCHK(svd_keep(c, ev, ord, QT, q, qp, tmp, B));
  if (left) {
    PMFCHK(rowgemm<EPI_STORE>(c, c->dV, c->np, c->np, B, c->np, nullptr, nullptr, c->dSvdP));
  } else {
    const int64_t total = c->mp * KP;
    hipLaunchKernelGGL(k_svd_w, dim3(elem_grid(total)), dim3(256), 0, c->stream, (const double*)c->dSvdE, qp, (const float*)nullptr, 1, c->m, total, KP,
                       r, (const double*)c->dSvdS, 1, c->dW);
    HIPCHK(c, hipGetLastError());
    w_replaced(c, false);
    PMFCHK(ensure_ps(c));
    HIPCHK(c, hipMemcpy2DAsync(c->dSvdP, (size_t)c->np * sizeof(float), c->dPS, ((size_t)c->np + KP) * sizeof(float),
                               (size_t)c->np * sizeof(float), (size_t)KP, hipMemcpyDeviceToDevice, c->stream));
    c->have_w = false;                                   // (U S^-1 is an operand, not a factor anybody asked for)
    c->ps_valid = false;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));           // the temporaries are released on return
  c->svd_rank = r; c->svd_left = left; c->svd_valid = true;
  return PMF_OK;
}

// dW <- the leading kb columns of U (float32)
int svd_load_w(pmf_ctx* c, int kb) {
  const int64_t total = c->mp * c->KP;
  hipLaunchKernelGGL(k_svd_w, dim3(elem_grid(total)), dim3(256), 0, c->stream, (const double*)c->dSvdE, (int)c->mp, (const float*)c->dSvdP,
                     c->svd_left ? 0 : 1, c->m, total, c->KP, kb, (const double*)c->dSvdS, 0, c->dW);
  HIPCHK(c, hipGetLastError());
  w_replaced(c, false);
  return PMF_OK;
}

// pmf_svd_decompose: svd_dense, then W = U and H = S V, so that pmf_frobenius is ||data - U S V|| (svd.py:92-107)
int svd_decompose(pmf_ctx* c) {
  if (svd_csr(c)) return svd_csr_decompose(c);
  PMFCHK(svd_dense(c));
  PMFCHK(svd_load_w(c, c->svd_rank));
  const int64_t total = (int64_t)c->KP * c->np;
  hipLaunchKernelGGL(k_svd_h, dim3(elem_grid(total)), dim3(256), 0, c->stream, c->svd_left ? (const double*)c->dSvdE : (const double*)nullptr,
                     (const float*)c->dSvdP, (int64_t)c->np, c->np, (int)c->n, c->svd_rank, total, (const double*)c->dSvdS, c->dH);
  HIPCHK(c, hipGetLastError());
  h_replaced(c, false, true);
  return PMF_OK;
}

// PCA.update_w (pca.py:93-108): W = the leading num_bases columns of U (all of them when num_bases == 0); S is descending
// already, so pca.py's argsort is the identity
int pca_update_w(pmf_ctx* c) {
  if (svd_csr(c)) return svd_csr_update_w(c);
  PMFCHK(svd_dense(c));
  const int kb = c->pca_bases > 0 ? std::min(c->pca_bases, c->svd_rank) : c->svd_rank;
  return svd_load_w(c, kb);
}

// PCA.update_h (pca.py:90-91): H = W^T data
int pca_update_h(pmf_ctx* c) {
  if (svd_csr(c)) return svd_csr_update_h(c);
  PMFCHK(ensure_ps(c));
  HIPCHK(c, hipMemcpy2DAsync(c->dH, (size_t)c->np * sizeof(float), c->dPS, ((size_t)c->np + c->KP) * sizeof(float),
                             (size_t)c->np * sizeof(float), (size_t)c->KP, hipMemcpyDeviceToDevice, c->stream));
  h_replaced(c, false, true);
  return PMF_OK;
}

// ||data - W H||: the direct residual (a full-rank PCA fits exactly: the trace identity would cancel)
int pca_error(pmf_ctx* c, double* out) {
  if (svd_csr(c)) return svd_csr_error(c, out);
  if (c->nb == 1) return frobenius_direct(c, out);
  PMFCHK(resid_bigk(c, false, c->dScal));
  double ss = 0.0;
  HIPCHK(c, hipMemcpyAsync(&ss, c->dScal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out = std::sqrt(ss);
  return PMF_OK;
}

// U (rows x r), S (r) and V (r x cols) of the last svd_dense as float64, row-major; any of them may be null
int svd_get(pmf_ctx* c, double* U, double* S, double* V) {
  if (svd_csr(c)) return svd_csr_get(c, U, S, V);
  if (!c->svd_valid) return fail(c, PMF_EINVAL, "pmf_svd_get: no decomposition of the current data (pmf_svd_decompose / pmf_update_w first)");
  const int r = c->svd_rank, KP = c->KP;
  const int64_t m = c->m, n = c->n;
  const int qp = c->svd_left ? c->np : (int)c->mp;
  if (r == 0) return PMF_OK;
  if (S) HIPCHK(c, hipMemcpyAsync(S, c->dSvdS, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  std::vector<double> E;
  std::vector<float> P;
  if ((c->svd_left && V) || (!c->svd_left && U)) {
    E.resize((size_t)r * qp);
    HIPCHK(c, hipMemcpyAsync(E.data(), c->dSvdE, E.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  if ((c->svd_left && U) || (!c->svd_left && V)) {
    P.resize(c->svd_left ? (size_t)m * KP : (size_t)r * c->np);
    HIPCHK(c, hipMemcpyAsync(P.data(), c->dSvdP, P.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->svd_left) {
    if (V) for (int i = 0; i < r; ++i) std::memcpy(V + (size_t)i * n, E.data() + (size_t)i * qp, (size_t)n * sizeof(double));
    if (U) for (int64_t row = 0; row < m; ++row) for (int i = 0; i < r; ++i) U[(size_t)row * r + i] = (double)P[(size_t)row * KP + i];
  } else {
    if (U) for (int64_t row = 0; row < m; ++row) for (int i = 0; i < r; ++i) U[(size_t)row * r + i] = E[(size_t)i * qp + row];
    if (V) for (int i = 0; i < r; ++i) for (int64_t col = 0; col < n; ++col) V[(size_t)i * n + col] = (double)P[(size_t)i * c->np + col];
  }
  return PMF_OK;
}

}  // namespace
