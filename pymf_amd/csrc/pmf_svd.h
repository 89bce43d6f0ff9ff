// pmf_svd.h -- SVD / PCA (pymf/svd.py:110-158, pymf/pca.py): the float64 Gram matrix of the resident float32 V and the small
// kernels that turn its eigenpairs into U, S, V.
//
// svd.py takes the SVD of the data through the eigen-decomposition of the Gram matrix on the SHORT side (data^T data for
// rows > cols, data data^T otherwise), drops eigenvalues <= 1e-8 (absolute) and divides by the square roots of the rest.
// A Gram matrix summed in float32 carries 1e-7 lambda_max of noise in every entry: a null eigenvalue (centred data with
// rows > cols always has one) can pass the cut and come back as a singular triple scaled by 1 / sqrt(noise).  So the Gram
// matrix is formed in float64: operands widened on load (exact), products (exact: 48 bits) and sums on the float64 MFMA.
#pragma once
#include "pmf_dev.h"

constexpr int PMF_SVD_TILE = 64;            // a workgroup owns a 64 x 64 tile of the Gram matrix ...
constexpr int PMF_SVD_MIN_CHUNK = 512;      // ... and at least this much of the inner dimension (a multiple of 64)
constexpr int PMF_SVD_TARGET_WGS = 512;     // tiles x chunks aimed at
constexpr int PMF_SVD_MAX_RANK = 2432;      // min(rows, cols): the Jacobi limit is 4096, the product paths carry 2432 bases

// Tile t of a product's tile grid -> (block row, block column).  SYM: the upper block triangle of a T x T grid, row by row
// (row <= column); otherwise the full grid with T tile columns.
template <bool SYM>
__device__ __forceinline__ int2 prod_tile(int t, int T) {
  if constexpr (!SYM) return make_int2(t / T, t % T);
  int ti = 0;
  while (t >= T - ti) { t -= T - ti; ++ti; }
  return make_int2(ti, ti + t);
}

// Partial 64 x 64 tile of a float64 product of two float32 operands, zero padded to whole tiles and widened on load:
//   TRANS = false: O [ra][rb] = sum_k A[ra][k] B[rb][k];   TRANS = true: O [ra][rb] = sum_k A[k][ra] B[k][rb].
// SYM = true is a Gram matrix (A == B, lda == ldb: V V^T or V^T V of SVD / PCA, Cg^T Cg and Rg Rg^T of CUR), of which the upper
// block triangle is formed; SYM = false the cross product of CUR (T = V Rg^T or T' = Cg^T V) on the full TA x TB grid.
// grid = (tiles in prod_tile's order, chunks of the inner dimension), 256 threads: wave w owns rows 16 w .. 16 w + 15 of the
// tile, four 16 x 16 accumulators (the four column blocks).
// Operand order of v_mfma_f64_16x16x4_f64 (pmf_inv.h: tile_dgemm): lane l supplies row / column l & 15 at k = l >> 4.
//   TRANS = false: both operands are contiguous along k.  Lane (i, g) fetches the four consecutive values k0 + 4 g .. + 3 of its
//     row with one 16-byte load and feeds value u to MFMA step u: step u sums k0 + 4 g + u over g -- the same set for both
//     operands, and the order of k inside a sum is free.
//   TRANS = true: the lanes of one MFMA row (equal g) read 16 adjacent columns of row k0 + 4 s + g.
// slab [chunk][tile][64][64] float64: no atomics, the chunks are added in a fixed order by k_prod_reduce_f64.
// chunk_len and inner are multiples of 64.
template <bool TRANS, bool SYM>
__global__ __launch_bounds__(256) void k_prod_f64(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                  int inner, int chunk_len, int TB, double* __restrict__ slab) {
  const int2 tl = prod_tile<SYM>((int)blockIdx.x, TB);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int k0 = (int)blockIdx.y * chunk_len;
  const int k1 = k0 + chunk_len < inner ? k0 + chunk_len : inner;
  const int ra = tl.x * PMF_SVD_TILE + wv * 16 + i;   // the A operand's row of the output
  const int rb = tl.y * PMF_SVD_TILE + i;             // the B operand's: rb + 16 j
  f64x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  if constexpr (!TRANS) {
    const float* ap = A + (int64_t)ra * lda + 4 * g;
    const float* bp = B + (int64_t)rb * ldb + 4 * g;
    for (int k = k0; k < k1; k += 32) {
      f32x4 a[2], b[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        a[h] = *reinterpret_cast<const f32x4*>(ap + k + 16 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = *reinterpret_cast<const f32x4*>(bp + (int64_t)(16 * j) * ldb + k + 16 * h);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = mfma_f64((double)a[h][u], (double)b[h][j][u], acc[j]);
    }
  } else {
    const float* ap = A + (int64_t)g * lda + ra;
    const float* bp = B + (int64_t)g * ldb + rb;
    for (int k = k0; k < k1; k += 16) {
      float a[4], b[4][4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        a[s] = ap[(int64_t)(k + 4 * s) * lda];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[s][j] = bp[(int64_t)(k + 4 * s) * ldb + 16 * j];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma_f64((double)a[s], (double)b[s][j], acc[j]);
    }
  }
  // C / D layout: lane l, register r <-> row (l >> 4) + 4 r, column l & 15
  double* o = slab + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (PMF_SVD_TILE * PMF_SVD_TILE);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(wv * 16 + g + 4 * r) * PMF_SVD_TILE + 16 * j + i] = acc[j][r];
}

// The sum of cnt partials p[0], p[stride], ... in a fixed order, one sum per lane of a 1024-thread workgroup: wave w adds
// partials w, w + 16, ..., the 16 sums are combined in wave order through part (as k_reduce_slabs_block); every wave returns the sum.
__device__ __forceinline__ double sum_partials16(const double* __restrict__ p, int64_t stride, int cnt, double (*part)[64]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double s = 0.0;
#pragma unroll 4
  for (int q = wv; q < cnt; q += 16) s += p[q * stride];
  part[wv][lane] = s;
  __syncthreads();
  double tot = part[0][lane];
#pragma unroll
  for (int w = 1; w < 16; ++w) tot += part[w][lane];
  return tot;
}

// Tile (ta, tb) of O [.][ld] (prod_tile's order, as k_prod_f64) = the sum of its nchunks partial tiles.
// grid = ntiles * 64 (64 elements per workgroup), 1024 threads.
template <bool SYM>
__global__ __launch_bounds__(1024) void k_prod_reduce_f64(const double* __restrict__ slab, int nchunks, int ntiles, int TB,
                                                          double* __restrict__ O, int64_t ld) {
  __shared__ double part[16][64];
  const int tile = (int)blockIdx.x >> 6;
  const int e = (((int)blockIdx.x & 63) << 6) + (threadIdx.x & 63);       // element of the tile
  const double tot = sum_partials16(slab + (int64_t)tile * (PMF_SVD_TILE * PMF_SVD_TILE) + e,
                                    (int64_t)ntiles * (PMF_SVD_TILE * PMF_SVD_TILE), nchunks, part);
  if (threadIdx.x < 64) {
    const int2 tl = prod_tile<SYM>(tile, TB);
    O[((int64_t)tl.x * PMF_SVD_TILE + (e >> 6)) * ld + tl.y * PMF_SVD_TILE + (e & 63)] = tot;
  }
}

// The kept eigenpairs in descending order: E [KP][ld] float64, row i = row order[i] of QT (columns >= q and rows >= r zero), and
// B [KP][ld] float32, row i = that row / s_i (the operand of the projection).  Either may be null.
__global__ __launch_bounds__(256) void k_svd_gather(const double* __restrict__ QT, int ld, int q, int r, int KP,
                                                    const int* __restrict__ order, const double* __restrict__ sv,
                                                    double* __restrict__ E, float* __restrict__ B) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)KP * ld) return;
  const int i = (int)(idx / ld), c = (int)(idx % ld);
  double v = 0.0;
  if (i < r && c < q) v = QT[(int64_t)order[i] * ld + c];
  if (E) E[idx] = v;
  if (B) B[idx] = i < r ? (float)(v / sv[i]) : 0.f;
}

// W [mp][KP] float32 <- the leading kb columns of U, scaled (inv_s != 0: u_i / s_i, the operand of V = S^-1 U^T data) or not;
// U's column i is row i of E (float64, eigenvector side: `right`) or column i of P [mp][KP] float32 (projected side).
__global__ __launch_bounds__(256) void k_svd_w(const double* __restrict__ E, int lde, const float* __restrict__ P, int right, int64_t m,
                                               int64_t total, int KP, int kb, const double* __restrict__ sv, int inv_s,
                                               float* __restrict__ W) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / KP;
    const int i = (int)(idx % KP);
    float o = 0.f;
    if (row < m && i < kb) {
      const double u = right ? E[(int64_t)i * lde + row] : (double)P[idx];
      o = (float)(inv_s ? u / sv[i] : u);
    }
    W[idx] = o;
  }
}

// H [KP][np] float32 <- diag(S) V: row i of V is row i of P [.][ldp] float32 (projected side) or of E [KP][np] float64
__global__ __launch_bounds__(256) void k_svd_h(const double* __restrict__ E, const float* __restrict__ P, int64_t ldp, int np, int n,
                                               int r, int64_t total, const double* __restrict__ sv, float* __restrict__ H) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int i = (int)(idx / np), c = (int)(idx % np);
    float o = 0.f;
    if (i < r && c < n) o = (float)(sv[i] * (E ? E[idx] : (double)P[(int64_t)i * ldp + c]));
    H[idx] = o;
  }
}
