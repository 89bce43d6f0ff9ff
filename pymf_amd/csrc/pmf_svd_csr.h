// pmf_svd_csr.h -- SVD / PCA on CSR data (the reference's sparse branch of svd.py:160-244): the projected side of the decomposition,
// PCA's H = W^T data and the cross term of the error as one pass over stored entries, and the float64 sums of the error identity.
// No dense V exists on such a context.
//
// Arrays: the CSR image of V and of V^T as CUR / CMD keep them (pmf_cur_csr.h): indptr [lines_p + 1] int64 with the pad lines empty,
// indices [nnz] int32 strictly ascending within a line, vals [nnz] float32.  A stored zero is a zero.
//
// k_csr_proj_f64   Out [lines_p][ldo] float64, Out[line][c] = sum over the entries (j, v) of the line of v * B[j][c] for the columns
//                  c of panel blockIdx.y (64 columns; B [.][ldb] float64, its pad columns zero): 256 threads, a wave owns whole lines
//                  (PMF_PROJ_LPW of them, lines 4 j + wave of the workgroup's 4 PMF_PROJ_LPW), lane <-> column, so an entry costs one
//                  contiguous 512-byte read of a row of B.  The wave loads 64 entries of the line in one coalesced read and hands
//                  them round by v_readlane, four at a time: the four rows of B are independent loads, in flight together.  Entry e
//                  of the line is added to accumulator e mod 4 in line order, the line's sum is (a0 + a1) + (a2 + a3): the order
//                  follows from the line's length alone.  Products are exact in float64 (24 x 53 bits round once in the fma).  An
//                  empty line and a pad line give exactly 0.  No atomics, no LDS, no private segment.
// k_svd_csr_b      B [qp][rp] float64 = the kept eigenvectors by columns, scaled: column i = row i of E [.][lde] times 1 / s_i (the
//                  operand of the projection), s_i (the scaled factor of the error) or 1; rows >= q and columns >= r zero.
// k_svd_csr_cols   Wd [rows_p][wp] float64 = the leading kb columns of P [rows_p][rp] (rows >= rows zero, columns >= kb zero).
// k_tsgram_f64     part [chunk][wp][wp] float64 = X^T Y over the rows of chunk `chunk` (X, Y [rows_p][ld] float64): grid = (wp / 16,
//                  wp / 16, chunks), 256 threads = one 16 x 16 tile, 32 rows staged in LDS at a time, each thread adds its products in
//                  row order.  k_tsgram_reduce_f64 adds the chunks in chunk order.
// k_dot_f64        part [block] = sum of x[e] * y[e] over the block's contiguous range (a thread adds its elements t, t + 256, ...
//                  in order, the workgroup's sums meet in an LDS tree): the host adds the blocks in block order.
// The order of every sum is fixed by the launch shape, which follows from the data's shape and the kept count alone.
#pragma once
#include "pmf_dev.h"

constexpr int PMF_PROJ_LPW = 4;             // lines a wave of k_csr_proj_f64 takes
constexpr int PMF_PROJ_LINES = 4 * PMF_PROJ_LPW;   // ... and a workgroup
constexpr int PMF_TSGRAM_ROWS = 32;         // rows of X and Y that k_tsgram_f64 stages at a time
constexpr int PMF_DOT_BLOCKS = 256;         // workgroups of k_dot_f64 at most

__global__ __launch_bounds__(256) void k_csr_proj_f64(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const float* __restrict__ vals, int64_t lines_p, const double* __restrict__ B,
                                                      int ldb, double* __restrict__ Out, int ldo) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = (int)blockIdx.y * 64 + lane;
  const double* Bc = B + col;
#pragma unroll 1
  for (int j = 0; j < PMF_PROJ_LPW; ++j) {
    const int64_t line = (int64_t)blockIdx.x * PMF_PROJ_LINES + 4 * j + wv;
    if (line >= lines_p) break;                   // (uniform over the wave)
    const int64_t hi = indptr[line + 1];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int64_t f0 = indptr[line]; f0 < hi; f0 += 64) {
      const int cnt = (int)(hi - f0 < 64 ? hi - f0 : 64);
      const int my_i = lane < cnt ? indices[f0 + lane] : 0;
      const int my_v = lane < cnt ? __float_as_int(vals[f0 + lane]) : 0;
      int s = 0;
      for (; s + 4 <= cnt; s += 4) {
        const int i0 = __builtin_amdgcn_readlane(my_i, s), i1 = __builtin_amdgcn_readlane(my_i, s + 1);
        const int i2 = __builtin_amdgcn_readlane(my_i, s + 2), i3 = __builtin_amdgcn_readlane(my_i, s + 3);
        const double b0 = Bc[(int64_t)i0 * ldb], b1 = Bc[(int64_t)i1 * ldb], b2 = Bc[(int64_t)i2 * ldb], b3 = Bc[(int64_t)i3 * ldb];
        a0 = fma((double)__int_as_float(__builtin_amdgcn_readlane(my_v, s)), b0, a0);
        a1 = fma((double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 1)), b1, a1);
        a2 = fma((double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 2)), b2, a2);
        a3 = fma((double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 3)), b3, a3);
      }
      if (s < cnt) {                              // the last one to three entries of the line (s is a multiple of 4)
        const int i0 = __builtin_amdgcn_readlane(my_i, s);
        const int i1 = __builtin_amdgcn_readlane(my_i, s + 1 < cnt ? s + 1 : s), i2 = __builtin_amdgcn_readlane(my_i, s + 2 < cnt ? s + 2 : s);
        const double b0 = Bc[(int64_t)i0 * ldb], b1 = Bc[(int64_t)i1 * ldb], b2 = Bc[(int64_t)i2 * ldb];
        a0 = fma((double)__int_as_float(__builtin_amdgcn_readlane(my_v, s)), b0, a0);
        if (s + 1 < cnt) a1 = fma((double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 1)), b1, a1);
        if (s + 2 < cnt) a2 = fma((double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 2)), b2, a2);
      }
    }
    Out[line * ldo + col] = (a0 + a1) + (a2 + a3);
  }
}

// mode 0: 1 / s_i, 1: s_i, 2: unscaled
__global__ __launch_bounds__(256) void k_svd_csr_b(const double* __restrict__ E, int lde, int q, int qp, int r, int rp,
                                                   const double* __restrict__ sv, int mode, double* __restrict__ B) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)qp * rp) return;
  const int c = (int)(idx / rp), i = (int)(idx % rp);
  double v = 0.0;
  if (i < r && c < q) {
    v = E[(int64_t)i * lde + c];
    if (mode == 0) v /= sv[i];
    if (mode == 1) v *= sv[i];
  }
  B[idx] = v;
}

__global__ __launch_bounds__(256) void k_svd_csr_cols(const double* __restrict__ P, int rp, int64_t rows, int64_t total, int kb, int wp,
                                                      double* __restrict__ Wd) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / wp;
    const int i = (int)(idx % wp);
    Wd[idx] = row < rows && i < kb ? P[row * rp + i] : 0.0;
  }
}

__global__ __launch_bounds__(256) void k_tsgram_f64(const double* __restrict__ X, const double* __restrict__ Y, int ld, int64_t rows_p,
                                                    int64_t chunk_len, int wp, double* __restrict__ part) {
  __shared__ double sX[PMF_TSGRAM_ROWS][16], sY[PMF_TSGRAM_ROWS][16];
  const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
  const int a0 = (int)blockIdx.x * 16, b0 = (int)blockIdx.y * 16;
  const int64_t lo = (int64_t)blockIdx.z * chunk_len;
  const int64_t hi = lo + chunk_len < rows_p ? lo + chunk_len : rows_p;     // (both multiples of PMF_TSGRAM_ROWS: the host sees to it)
  double s = 0.0;
  for (int64_t r0 = lo; r0 < hi; r0 += PMF_TSGRAM_ROWS) {
#pragma unroll
    for (int h = 0; h < PMF_TSGRAM_ROWS / 16; ++h) {
      const int rr = 16 * h + a;
      sX[rr][b] = X[(r0 + rr) * ld + a0 + b];
      sY[rr][b] = Y[(r0 + rr) * ld + b0 + b];
    }
    __syncthreads();
#pragma unroll 8
    for (int rr = 0; rr < PMF_TSGRAM_ROWS; ++rr) s = fma(sX[rr][a], sY[rr][b], s);
    __syncthreads();
  }
  part[(int64_t)blockIdx.z * wp * wp + (int64_t)(a0 + a) * wp + b0 + b] = s;
}

__global__ __launch_bounds__(256) void k_tsgram_reduce_f64(const double* __restrict__ part, int nchunks, int64_t elems, double* __restrict__ G) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  double s = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) s += part[(int64_t)ch * elems + e];
  G[e] = s;
}

__global__ __launch_bounds__(256) void k_dot_f64(const double* __restrict__ x, const double* __restrict__ y, int64_t n, int64_t per_block,
                                                 double* __restrict__ part) {
  __shared__ double red[256];
  const int64_t lo = (int64_t)blockIdx.x * per_block;
  const int64_t hi = lo + per_block < n ? lo + per_block : n;
  double s = 0.0;
  for (int64_t e = lo + threadIdx.x; e < hi; e += 256) s = fma(x[e], y[e], s);
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
