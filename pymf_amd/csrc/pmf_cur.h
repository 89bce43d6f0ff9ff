// pmf_cur.h -- CUR / CMD (pymf/cur.py, pymf/cmd.py): the sampling norms of the resident float32 V, the gather of the chosen
// columns and rows, and the factors.  The one product that touches the whole data, T = V Rg^T or T' = Cg^T V, is k_prod_f64 of
// pmf_svd.h on the full tile grid.
//
// cur.py:99-120 computes U = pinv(C) data pinv(R) with C = data[:, cid] diag(sqrt(ccnt)), R = diag(sqrt(rcnt)) data[rid, :].
// With Cg, Rg the unscaled gathers and dc = sqrt(ccnt), dr = sqrt(rcnt) this is
//   U = (C^T C)^+ (dc o (Cg^T data Rg^T) o dr) (R R^T)^+ ,   C^T C = dc dc^T o (Cg^T Cg),   R R^T = dr dr^T o (Rg Rg^T).
// A pseudo-inverse sits on either side of the middle product, so it is formed by the kernel of the Gram matrices: operands
// widened on load (exact), products (exact: 48 bits) and sums on the float64 MFMA, the chunks of the inner dimension added in a
// fixed order.  A float32 middle product is off by 2e-5 ... 2e-3 of max |U| on well-conditioned cases already.
#pragma once
#include "pmf_dev.h"
#include "pmf_svd.h"

constexpr int PMF_CUR_MAX_RANK = 128;       // rows / columns sampled: two 64-wide tiles of k_prod_f64, one KP = 128 block of W and H
constexpr int PMF_CUR_PANEL = 256;          // columns a workgroup of k_cur_sqnorms owns (four 64-column sub-panels)

// Row and column sums of squares of V [mp][ld] float32 (zero padded), float64.  grid = blocks of 64 rows x npanels panels of 256
// columns (block index = row block * npanels + panel), 256 threads.  Wave w owns rows 16 w .. 16 w + 15 of the block and walks the panel's sub-panels of 64 columns: lane (i, g)
// loads the four columns 4 i .. 4 i + 3 of row 4 s + g with one 16-byte load.  A row's sum is reduced over the 16 lanes of its
// g by a butterfly, a column's over the four g and then, through LDS, over the four waves in wave order.
//   rowpart [panel][mp], colpart [row block][ld]: no atomics, k_cur_sqnorms_reduce adds them in a fixed order.
__global__ __launch_bounds__(256) void k_cur_sqnorms(const float* __restrict__ V, int64_t ld, int64_t mp, int npanels,
                                                     double* __restrict__ rowpart, double* __restrict__ colpart) {
  __shared__ double part[4][PMF_CUR_PANEL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int panel = (int)(blockIdx.x % (unsigned)npanels), rblk = (int)(blockIdx.x / (unsigned)npanels);
  const int64_t c0 = (int64_t)panel * PMF_CUR_PANEL;
  const int64_t r0 = (int64_t)rblk * 64 + 16 * wv;
  const int nsub = (int)((ld - c0 < PMF_CUR_PANEL ? ld - c0 : PMF_CUR_PANEL) / 64);   // ld is a multiple of 64
  double rs[4] = {0.0, 0.0, 0.0, 0.0};
  double cs[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int e = 0; e < 4; ++e) cs[p][e] = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (p < nsub) {
      f32x4 x[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) x[s] = *reinterpret_cast<const f32x4*>(V + (r0 + 4 * s + g) * ld + c0 + 64 * p + 4 * i);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        double q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { q[e] = (double)x[s][e] * (double)x[s][e]; cs[p][e] += q[e]; }
        rs[s] += (q[0] + q[1]) + (q[2] + q[3]);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) rs[s] += __shfl_xor(rs[s], d);
    if (i == 0) rowpart[(int64_t)panel * mp + r0 + 4 * s + g] = rs[s];
  }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double v = cs[p][e];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (g == 0) part[wv][64 * p + 4 * i + e] = v;
    }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 64 * nsub) colpart[(int64_t)rblk * ld + c0 + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
}

// out [mp + ld]: the row sums (over the npanels partials of rowpart), then the column sums (over the nblocks partials of colpart),
// each in the fixed order of sum_partials16 (pmf_svd.h).  64 outputs per workgroup of 1024 threads, grid = (mp + ld) / 64.
__global__ __launch_bounds__(1024) void k_cur_sqnorms_reduce(const double* __restrict__ rowpart, int npanels, int64_t mp,
                                                             const double* __restrict__ colpart, int nblocks, int64_t ld,
                                                             double* __restrict__ out) {
  __shared__ double part[16][64];
  const int64_t e = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const bool row = e < mp;
  const double tot = sum_partials16(row ? rowpart + e : colpart + (e - mp), row ? mp : ld, row ? npanels : nblocks, part);
  if (threadIdx.x < 64) out[e] = tot;
}

// The chosen columns and rows of V [mp][np], unscaled: Cg [mp][cp] (column j = column cid[j] of V, columns >= nc zero) and
// Rg [rp][np] (row i = row rid[i] of V, rows >= nr zero); the indices are in range (the host checks).  The side that meets the
// float64 intermediate in the second, small product is also written widened: CgT [cp][mp] (rows <= cols) or Rd [rp][np].
__global__ __launch_bounds__(256) void k_cur_gather(const float* __restrict__ V, int64_t mp, int np, const int* __restrict__ cid, int nc,
                                                    int cp, const int* __restrict__ rid, int nr, int rp, float* __restrict__ Cg,
                                                    float* __restrict__ Rg, double* __restrict__ CgT, double* __restrict__ Rd) {
  const int64_t nC = mp * cp, total = nC + (int64_t)rp * np;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    if (idx < nC) {
      const int64_t row = idx / cp;
      const int j = (int)(idx % cp);
      const float v = j < nc ? V[row * np + cid[j]] : 0.f;
      Cg[idx] = v;
      if (CgT) CgT[(int64_t)j * mp + row] = (double)v;
    } else {
      const int64_t q = idx - nC;
      const int i = (int)(q / np), col = (int)(q % np);
      const float v = i < nr ? V[(int64_t)rid[i] * np + col] : 0.f;
      Rg[q] = v;
      if (Rd) Rd[q] = (double)v;
    }
  }
}

// A [i][j] *= d[i] d[j] for i, j < n: C^T C = dc dc^T o (Cg^T Cg), R R^T = dr dr^T o (Rg Rg^T)
__global__ __launch_bounds__(256) void k_cur_scale_sym(double* __restrict__ A, int ld, int n, const double* __restrict__ d) {
  const int q = (int)blockIdx.x * 256 + threadIdx.x;
  if (q >= n * n) return;
  const int i = q / n, j = q % n;
  A[(int64_t)i * ld + j] *= d[i] * d[j];
}

// The factors of the error ||data - C U R||: W [mp][KP] float32 <- C U = Cg (dc o U), the sum over the nc columns in float64 and
// one rounding (Us [nc][nr] = diag(dc) U, float64), and H [KP][np] float32 <- R = diag(dr) Rg; rows >= m, columns >= nr of W and
// rows >= nr of H are zero.
__global__ __launch_bounds__(256) void k_cur_factors(const float* __restrict__ Cg, int cp, int nc, const double* __restrict__ Us, int nr,
                                                     int64_t m, int64_t mp, int KP, const float* __restrict__ Rg, int np,
                                                     const double* __restrict__ dr, float* __restrict__ W, float* __restrict__ H) {
  const int64_t nW = mp * KP, total = nW + (int64_t)KP * np;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    if (idx < nW) {
      const int64_t row = idx / KP;
      const int j = (int)(idx % KP);
      double s = 0.0;
      if (row < m && j < nr) {
        const float* cr = Cg + row * cp;
        for (int q = 0; q < nc; ++q) s += (double)cr[q] * Us[(int64_t)q * nr + j];
      }
      W[idx] = (float)s;
    } else {
      const int64_t q = idx - nW;
      const int i = (int)(q / np);
      H[q] = i < nr ? (float)(dr[i] * (double)Rg[q]) : 0.f;
    }
  }
}
