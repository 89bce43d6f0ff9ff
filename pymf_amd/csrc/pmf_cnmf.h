// pmf_cnmf.h -- convex NMF (Ding, Li, Jordan; pymf/cnmf.py:108-187) and its k-means initialisation (pymf/kmeans.py:64-87,
// pymf/cnmf.py:78-103) in Gram space.
//
// Every quantity the reference's CNMF loop touches is a product with C = V^T V (n x n, formed once by ensure_vgram) or a
// k x k / n x k matrix: W = V G is only ever READ (frobenius_norm) and is materialised on demand.  All of it is float64 on the
// float64 MFMA (v_mfma_f64_16x16x4_f64, the operand layouts of tile_dgemm in pmf_inv.h).  Layouts:
//   C            [np][np]   symmetric, zero beyond n
//   every n x k matrix is held TRANSPOSED, k x n like H: G^T, the k-means coefficients Z^T, (neg(C) X)^T, (pos(C) X)^T
//   [KP][np], zero beyond (k, n);  k x k matrices [KP][KP].
// Kernels that run inside pmf_factorize's free-running loop take the stop flag (dStop) and return at once when it is raised.
#pragma once
#include "pmf_dev.h"   // f64x4, mfma_f64
#include "pmf_inv.h"   // tile_dgemm

// (X^T neg(C), X^T pos(C)) = ((neg(C) X)^T, (pos(C) X)^T) for an n x k X given as XT [KP][np] (C is symmetric):
// pos(C) = (|C| + C) / 2, neg(C) = (|C| - C) / 2 (cnmf.py:139-152).  The C fragment is loaded once per k-step and split in
// registers; the two products run as two accumulator chains over the same loads.  grid = (np / 16, KP / 16), 64 threads.
__global__ __launch_bounds__(64) void k_cnmf_split_gemm(const double* __restrict__ XT, const double* __restrict__ C, int np,
                                                        double* __restrict__ YnT, double* __restrict__ YpT,
                                                        const int* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int lane = threadIdx.x, c0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const int i = lane & 15, g = lane >> 4;
  const double* ap = XT + (int64_t)(r0 + i) * np + g;          // A[r0 + i][4 s + g] = X^T
  const double* bp = C + (int64_t)g * np + c0 + i;             // B[4 s + g][c0 + i] = C
  f64x4 accp = {0.0, 0.0, 0.0, 0.0}, accn = {0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < np / 4; s0 += 16) {                     // np is a multiple of 64
    double a[16], b[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) { a[u] = ap[4 * (s0 + u)]; b[u] = bp[(int64_t)(s0 + u) * 4 * np]; }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const double cp = (fabs(b[u]) + b[u]) / 2.0;
      const double cn = (fabs(b[u]) - b[u]) / 2.0;
      accp = mfma_f64(a[u], cp, accp);
      accn = mfma_f64(a[u], cn, accn);
    }
  }
  const int col = c0 + i;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = r0 + g + 4 * r;
    YnT[row * np + col] = accn[r];
    YpT[row * np + col] = accp[r];
  }
}

// (L1 | L2) = (X1 Y^T | X2 Y^T), k x k, contraction over the np columns of X1, X2, Y [KP][np].  grid = (KP / 16, KP / 16, 2),
// 64 threads; blockIdx.z picks the product.  CNMF: L_A = A^T G, L_B = B^T G (the H step's right factors, cnmf.py:163-166,
// reassociated: H^T (G^T A) instead of (H^T G^T) A with its n x n intermediate).
__global__ __launch_bounds__(64) void k_cnmf_kxk2(const double* __restrict__ X1, const double* __restrict__ X2,
                                                  const double* __restrict__ Y, int np, int KP,
                                                  double* __restrict__ L1, double* __restrict__ L2, const int* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int lane = threadIdx.x, c0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const double* X = blockIdx.z == 0 ? X1 : X2;
  double* L = blockIdx.z == 0 ? L1 : L2;
  const f64x4 acc = tile_dgemm<true, double>(X, np, Y, np, np, r0, c0, lane);
  const int col = c0 + (lane & 15), g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) L[(int64_t)(r0 + g + 4 * r) * KP + col] = acc[r];
}

// The multiplicative sqrt rule of both CNMF steps, k x n (transposed) form, in place:
//   T <- T * sqrt( (P1 + L1 X1) / (P2 + L2 X2 + 1e-9) )
// H step (cnmf.py:162-167):  T = H,   P1 = (pos(C) G)^T, L1 = A^T G, X1 = H,   P2 = (neg(C) G)^T, L2 = B^T G, X2 = H
// G step (cnmf.py:169-174):  T = G^T, P1 = H pos(C),     L1 = H H^T, X1 = A^T, P2 = H neg(C),     L2 = H H^T, X2 = B^T
// (A = neg(C) G, B = pos(C) G of the G the iteration started with; the 1e-9 guard where the reference adds it).
// One workgroup per 16-column panel, NT waves: wave w owns rows 16 w .. 16 w + 15 and runs the two k x k products of its tile
// as two accumulator chains.  Every wave has read the panel before any writes it (the H step reads T itself as X1 = X2).
// Tf (may be null): the float32 rounding of the new T.  grid = np / 16, 64 NT threads.
template <int NT>
__global__ __launch_bounds__(64 * NT) void k_cnmf_mul_step(double* T /* in place, may alias X1 / X2: NOT restrict */,
                                                           float* __restrict__ Tf, int np,
                                                           const double* __restrict__ P1, const double* __restrict__ P2,
                                                           const double* __restrict__ L1, const double* __restrict__ L2,
                                                           const double* X1, const double* X2, const int* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  constexpr int KP = 16 * NT, KS = KP / 4;
  constexpr int RND = KS < 16 ? KS : 16;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int c0 = 16 * blockIdx.x, r0 = 16 * wv;
  double tv[4], p1[4], p2[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t e = (int64_t)(r0 + g + 4 * r) * np + c0 + i;
    tv[r] = T[e]; p1[r] = P1[e]; p2[r] = P2[e];
  }
  const double* a1 = L1 + (int64_t)(r0 + i) * KP + g;          // A[r0 + i][4 s + g]
  const double* a2 = L2 + (int64_t)(r0 + i) * KP + g;
  const double* b1 = X1 + (int64_t)g * np + c0 + i;             // B[4 s + g][c0 + i]
  const double* b2 = X2 + (int64_t)g * np + c0 + i;
  f64x4 acc1 = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s0 = 0; s0 < KS; s0 += RND) {
    double x1[RND], x2[RND], y1[RND], y2[RND];
#pragma unroll
    for (int u = 0; u < RND; ++u) {
      x1[u] = a1[4 * (s0 + u)]; x2[u] = a2[4 * (s0 + u)];
      y1[u] = b1[(int64_t)(s0 + u) * 4 * np]; y2[u] = b2[(int64_t)(s0 + u) * 4 * np];
    }
#pragma unroll
    for (int u = 0; u < RND; ++u) {
      acc1 = mfma_f64(x1[u], y1[u], acc1);
      acc2 = mfma_f64(x2[u], y2[u], acc2);
    }
  }
  __syncthreads();                                              // every wave has read the old panel
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t e = (int64_t)(r0 + g + 4 * r) * np + c0 + i;
    const double num = p1[r] + acc1[r];
    const double den = p2[r] + acc2[r] + 1e-9;
    const double tn = tv[r] * sqrt(num / den);
    T[e] = tn;
    if (Tf) Tf[e] = (float)tn;
  }
}

// Deterministic sum over one 1024-thread workgroup (fixed tree): the result in every thread.
__device__ __forceinline__ double cnmf_block_sum(double v, double* red /* [1024] LDS */) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// The two data-dependent terms of ||V - V G H||^2 = tr(C) - 2 <C G, H^T> + <G^T C G, H H^T> for the G at hand, from
// A = neg(C) G, B = pos(C) G (C G = B - A), L_A = A^T G, L_B = B^T G ((G^T C G)^T = L_B - L_A) and S = H H^T (symmetric):
//   tt[0] = <B^T - A^T, H>,   tt[1] = <L_B - L_A, S>          -> k_conv_check (pmf_small.h) with vnorm2 = tr(C).
// One workgroup of 1024 threads, fixed order.
__global__ __launch_bounds__(1024) void k_cnmf_err_terms(const double* __restrict__ AT, const double* __restrict__ BT,
                                                         const double* __restrict__ H, int64_t nkn,
                                                         const double* __restrict__ LA, const double* __restrict__ LB,
                                                         const double* __restrict__ S, int64_t nkk,
                                                         double* __restrict__ tt, const int* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  __shared__ double red[1024];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t e = threadIdx.x; e < nkn; e += 1024) s0 += (BT[e] - AT[e]) * H[e];
  for (int64_t e = threadIdx.x; e < nkk; e += 1024) s1 += (LB[e] - LA[e]) * S[e];
  s0 = cnmf_block_sum(s0, red);
  s1 = cnmf_block_sum(s1, red);
  if (threadIdx.x == 0) { tt[0] = s0; tt[1] = s1; }
}

// tr(C) -> out[0] (one workgroup of 1024 threads)
__global__ __launch_bounds__(1024) void k_cnmf_trace(const double* __restrict__ C, int np, double* __restrict__ out) {
  __shared__ double red[1024];
  double s = 0.0;
  for (int i = threadIdx.x; i < np; i += 1024) s += C[(int64_t)i * np + i];
  s = cnmf_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- k-means in Gram space (pymf/kmeans.py:64-87 under NMF.factorize, pymf/nmf.py:171-202) ------------------------------
// Centre j is c_j = V z_j with z_j the n-vector of coefficients (ZT [KP][np]); with CZ^T = Z^T C (k_dgemm_mfma):
//   ||x_i - c_j||^2 = C_ii - 2 (C Z)_ij + z_j^T C z_j.

// Z^T <- the selected samples: z_j = e_{sel[j]} (kmeans.py:69-74; sel sorted by the caller).  grid-stride over KP x np.
__global__ __launch_bounds__(256) void k_kmeans_seed(double* __restrict__ ZT, int np, int KP, int k, const int* __restrict__ sel) {
  const int64_t total = (int64_t)KP * np;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e / np), i = (int)(e - (int64_t)j * np);
    ZT[e] = (j < k && sel[j] == i) ? 1.0 : 0.0;
  }
}

// zcz[j] = z_j^T C z_j = <Z^T[j], (Z^T C)[j]>: one workgroup of 256 threads per centre, fixed order.
__global__ __launch_bounds__(256) void k_kmeans_zcz(const double* __restrict__ ZT, const double* __restrict__ CZT, int np,
                                                    double* __restrict__ zcz, const int* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  __shared__ double red[256];
  const int j = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < np; i += 256) s += ZT[(int64_t)j * np + i] * CZT[(int64_t)j * np + i];
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) zcz[j] = red[0];
}

// assigned[i] = argmin_j ||x_i - c_j|| (dist.vq, dist.py:126-130: the LOWEST j among ties, np.argmin), dmin[i] its squared
// distance.  One thread per sample.
__global__ __launch_bounds__(256) void k_kmeans_assign(const double* __restrict__ C, const double* __restrict__ CZT,
                                                       const double* __restrict__ zcz, int n, int np, int k,
                                                       int* __restrict__ assigned, double* __restrict__ dmin,
                                                       const int* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double cii = C[(int64_t)i * np + i];
  double best = 0.0;
  int arg = 0;
  for (int j = 0; j < k; ++j) {
    const double d = cii - 2.0 * CZT[(int64_t)j * np + i] + zcz[j];
    if (j == 0 || d < best) { best = d; arg = j; }
  }
  assigned[i] = arg;
  dmin[i] = best;
}

// The members per centre and the k-means error of this iteration, ferr[it] = ||data - W H|| = sqrt(sum_i min_j D_ij)
// (nmf.py:100-114 with W the centres and H the one-hot assignment), then the reference's early exit (nmf.py:134-139,198-202):
// it > 1 and |ferr[it] - ferr[it - 1]| / n < eps raises stop (stop[1] = it).  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void k_kmeans_reduce(const int* __restrict__ assigned, const double* __restrict__ dmin, int n,
                                                        int k, int* __restrict__ count, double* __restrict__ ferr, int it,
                                                        double eps, int* __restrict__ stop) {
  if (stop[0] != 0) return;
  __shared__ double red[1024];
  __shared__ int cnt[128];
  const int t = threadIdx.x;
  if (t < 128) cnt[t] = 0;
  __syncthreads();
  double s = 0.0;
  for (int i = t; i < n; i += 1024) {
    s += fmax(dmin[i], 0.0);                                    // (a sample that is itself a centre: 0 up to C's rounding)
    atomicAdd(&cnt[assigned[i]], 1);
  }
  s = cnmf_block_sum(s, red);                                   // (its barriers order the LDS counts too)
  if (t < k) count[t] = cnt[t];
  if (t == 0 && it >= 0) {                                      // (it < 0: the assignment of init_h, kmeans.py:66-67 -- counts only)
    const double f = sqrt(s);
    ferr[it] = f;
    if (it > 1 && fabs(f - ferr[it - 1]) / (double)n < eps) { stop[1] = it; stop[0] = 1; }
  }
}

// update_w (kmeans.py:83-87): centre j becomes the mean of its members -- z_j = onehot(members) / count -- only when it has
// more than one member; otherwise it stays.  grid-stride over KP x np.
__global__ __launch_bounds__(256) void k_kmeans_update(double* __restrict__ ZT, int n, int np, int k, const int* __restrict__ assigned,
                                                       const int* __restrict__ count, const int* __restrict__ stop) {
  if (stop[0] != 0) return;
  const int64_t total = (int64_t)k * np;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e / np), i = (int)(e - (int64_t)j * np);
    const int cj = count[j];
    if (cj > 1) ZT[e] = (i < n && assigned[i] == j) ? 1.0 / (double)cj : 0.0;
  }
}

// G (host n x k, row-major, staged on the device) <-> G^T [KP][np] with zero padding
__global__ __launch_bounds__(256) void k_cnmf_g_to_gt(const double* __restrict__ G, int n, int k, int np, int KP, double* __restrict__ GT) {
  const int64_t total = (int64_t)KP * np;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e / np), i = (int)(e - (int64_t)j * np);
    GT[e] = (j < k && i < n) ? G[(int64_t)i * k + j] : 0.0;
  }
}
__global__ __launch_bounds__(256) void k_cnmf_gt_to_g(const double* __restrict__ GT, int n, int k, int np, double* __restrict__ G) {
  const int64_t total = (int64_t)n * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / k), j = (int)(e - (int64_t)i * k);
    G[e] = GT[(int64_t)j * np + i];
  }
}

// CNMF.init_h (cnmf.py:88-100) from the final assignment: H = onehot^T + 0.2, G[i, :] = (onehot_i + 0.01) / count(assigned_i);
// Hd, its float32 rounding H and G^T, all [KP][np] with zero padding.  with_h / with_g: which of them to write.
__global__ __launch_bounds__(256) void k_cnmf_init_hg(const int* __restrict__ assigned, const int* __restrict__ count, int n, int np,
                                                      int KP, int k, double* __restrict__ Hd, float* __restrict__ H,
                                                      double* __restrict__ GT, int with_h, int with_g) {
  const int64_t total = (int64_t)KP * np;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e / np), i = (int)(e - (int64_t)j * np);
    const bool in = j < k && i < n;
    const double oh = (in && assigned[i] == j) ? 1.0 : 0.0;
    if (with_h) {
      const double h = in ? oh + 0.2 : 0.0;
      Hd[e] = h;
      H[e] = (float)h;
    }
    if (with_g) GT[e] = in ? (oh + 0.01) / (double)count[assigned[i]] : 0.0;
  }
}
