// pmf_lev.h -- CURSL (pymf/cursl.py): the statistical leverage scores of the resident float32 V in float64.
//
// cursl.py samples with p_j proportional to sum_{l < kk} V_svd[l][j]^2, the squared column norms of the leading kk right singular
// vectors (and the same of the data's transpose for the rows).  svd.py takes both decompositions from the Gram matrix on the
// short side of the data; with (lambda_l, e_l) its kept eigenpairs in descending order,
//   eigenvector side (length q = min(rows, cols)):  lev_i = sum_l e_l[i]^2                           (k_lev_eig)
//   long side:                                       lev_j = sum_l (e_l . x_j)^2 / lambda_l          (k_lev_f64)
// with x_j column j of the data (rows <= cols) or row j (rows > cols).  The reference writes S^-1 U^T data out, kk x n float64
// values that are squared, summed and dropped; k_lev_f64 forms a 16 x 16 tile of them in the accumulators of the float64 MFMA and
// squares and sums it there: V is read once, one double per position is written.
#pragma once
#include "pmf_dev.h"

constexpr int PMF_LEV_MAX_K = 128;          // singular vectors in a leverage: eight 16-row operand tiles
constexpr int PMF_LEV_PANEL = 256;          // long-side positions of a workgroup: 64 per wave

// The operand P = diag(1/s) E (row l = e_l / s_l; rows >= kk and columns >= q zero) is stored in the order the MFMA takes it:
//   Pm [piece][tile][step][lane],  piece = 64 values of the inner dimension, tile = 16 operand rows, step = one MFMA (4 inner values),
//   lane (i, g) = operand row 16 tile + i at inner index 64 piece + lev_inner<TRANS>(step, g)
// so that a piece is one contiguous block that goes to LDS with 16-byte copies and a wave reads its MFMA operand as 512 adjacent bytes.
// TRANS = true: step s sums inner values 4 s + g (four adjacent rows of V).  TRANS = false: a lane holds four adjacent inner values
// 16 S + 4 g + u of its row (one 16-byte load) and feeds value u to step 4 S + u, as k_prod_f64<false, .> does.
template <bool TRANS>
__host__ __device__ __forceinline__ int lev_inner(int step, int g) {
  return TRANS ? 4 * step + g : 16 * (step >> 2) + 4 * g + (step & 3);
}

// Pm (above) from the eigenvector rows QT [.][ld] (row order[l] = e_l), sv[l] = sqrt(lambda_l): nt tiles, qp / 64 pieces
template <bool TRANS>
__global__ __launch_bounds__(256) void k_lev_gather(const double* __restrict__ QT, int ld, int q, int kk, int nt,
                                                    const int* __restrict__ order, const double* __restrict__ sv,
                                                    int64_t total, double* __restrict__ Pm) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int lane = (int)(idx & 63), step = (int)((idx >> 6) & 15);
  const int tile = (int)((idx >> 10) % nt), piece = (int)((idx >> 10) / nt);
  const int l = 16 * tile + (lane & 15), col = 64 * piece + lev_inner<TRANS>(step, lane >> 4);
  Pm[idx] = (l < kk && col < q) ? QT[(int64_t)order[l] * ld + col] / sv[l] : 0.0;
}

// lev [i] = sum_{l < kk} e_l[i]^2 for i < q, l ascending: the leverage of the eigenvector side
__global__ __launch_bounds__(256) void k_lev_eig(const double* __restrict__ QT, int ld, int q, int kk, const int* __restrict__ order,
                                                 double* __restrict__ lev) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i >= q) return;
  double s = 0.0;
  for (int l = 0; l < kk; ++l) {
    const double e = QT[(int64_t)order[l] * ld + i];
    s += e * e;
  }
  lev[i] = s;
}

// lev [pos] = sum_{l < 16 NT} (sum_k P[l][k] x_pos[k])^2 over the long side of V [.][ld] float32 (zero padded to multiples of 64):
//   TRANS = true  (rows <= cols): positions are columns of V, the inner dimension its qp rows;
//   TRANS = false (rows > cols):  positions are rows of V, the inner dimension its qp columns.
// grid = ceil(lp / 256) workgroups of 256 threads, lp the padded long side.  Wave w owns positions 256 b + 64 w .. + 63 (a wave
// past lp only helps with the copies) and all NT operand tiles: NT x 4 accumulators of 16 x 16, four blocks of 16 positions.
//   TRANS = true:  lane (i, g) loads columns 4 i .. 4 i + 3 of row 64 piece + 4 s + g with one 16-byte load -- the 16 lanes of a g
//     read 256 adjacent bytes -- and value j belongs to block j: block j holds positions 4 i + j.
//   TRANS = false: lane (i, g) loads inner values 16 S + 4 g .. + 3 of row 16 j + i (block j) with one 16-byte load.
// The workgroup walks the whole inner dimension in pieces of 64: the piece's block of Pm goes to LDS (NT x 8 KiB), then 16 steps x
// NT tiles x 4 blocks of v_mfma_f64_16x16x4_f64 (operand order and C / D layout: pmf_svd.h).  V arrives a quarter piece (four
// steps, four 16-byte loads per lane) ahead of its use, the first quarter of the next piece under the last of this one.
// V is widened on load (exact), products (48 bits) and sums are float64.  Epilogue: D row = operand row, D column = position, so
// a lane holds four operand rows of one position per accumulator: it adds their squares over registers and tiles in index order,
// two __shfl_xor steps add the four g, and the lanes of g = 0 write.  No atomics, no slab: two runs give the same bits.
// Waves per SIMD the register budget is set for: 128 accumulator registers at NT = 4 leave room for two (<= 256 registers)
constexpr int lev_waves(int nt) { return nt <= 2 ? 3 : nt <= 4 ? 2 : 1; }

// quarter `qd` of the piece at k0: TRANS = true x[u] = row k0 + 16 qd + 4 u + g (step 4 qd + u, value j = block j);
// TRANS = false x[j] = inner values k0 + 16 qd + 4 g .. + 3 of the lane's row of block j (value u = step 4 qd + u)
template <bool TRANS>
__device__ __forceinline__ void lev_load_quarter(const float* __restrict__ vp, int64_t ld, int k0, int qd, f32x4 (&x)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (TRANS) x[e] = *reinterpret_cast<const f32x4*>(vp + (int64_t)(k0 + 16 * qd + 4 * e) * ld);
    else x[e] = *reinterpret_cast<const f32x4*>(vp + (int64_t)(16 * e) * ld + k0 + 16 * qd);
  }
}

template <bool TRANS, int NT>
__global__ __launch_bounds__(256, lev_waves(NT)) void k_lev_f64(const float* __restrict__ V, int64_t ld, const double* __restrict__ Pm, int qp,
                                                                int64_t lp, double* __restrict__ lev) {
  __shared__ __attribute__((aligned(16))) double Pl[NT * 1024];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t pos0 = (int64_t)blockIdx.x * PMF_LEV_PANEL + 64 * wv;
  const bool active = pos0 < lp;                        // lp is a multiple of 64: a wave is inside or outside as a whole
  f64x4 acc[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const float* vp = TRANS ? V + (int64_t)g * ld + pos0 + 4 * i : V + (pos0 + i) * ld + 4 * g;
  f32x4 x[2][4];
  if (active) lev_load_quarter<TRANS>(vp, ld, 0, 0, x[0]);
  for (int k0 = 0; k0 < qp; k0 += 64) {
    __syncthreads();                                    // the previous piece has been read
    {
      const double2* src = reinterpret_cast<const double2*>(Pm + (int64_t)(k0 >> 6) * (NT * 1024));
      double2* dst = reinterpret_cast<double2*>(Pl);
#pragma unroll
      for (int r = 0; r < 2 * NT; ++r) dst[r * 256 + threadIdx.x] = src[r * 256 + threadIdx.x];
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        if (qd < 3) lev_load_quarter<TRANS>(vp, ld, k0, qd + 1, x[(qd + 1) & 1]);
        else if (k0 + 64 < qp) lev_load_quarter<TRANS>(vp, ld, k0 + 64, 0, x[0]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const double a = Pl[(t * 16 + 4 * qd + u) * 64 + lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float v = TRANS ? x[qd & 1][u][j] : x[qd & 1][j][u];
              acc[t][j] = mfma_f64(a, (double)v, acc[t][j]);
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);              // LDS reads are not hoisted across quarters: at NT = 8 they would spill
      }
    }
  }
  if (!active) return;
  double out[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) s += acc[t][j][r] * acc[t][j][r];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    out[j] = s;
  }
  if (g == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) lev[pos0 + (TRANS ? 4 * i + j : 16 * j + i)] = out[j];
  }
}
