// pmf_greedy_csr.h -- GREEDY on CSR data (the reference's sparse branch of greedy.py:115-141, which subtracts a rank-one matrix from
// the data in every round and so holds a dense matrix from the second round on).  Here the data are read only (DESIGN.md 3.16,
// 3.26): the score of pmf_greedy.h, T_j = |B'^T v_j|^2 / (|v_j|^2 - |Q^T v_j|^2), over stored entries.  No dense V exists on such a
// context.
//
// Arrays: the CSR image of V and of V^T as CUR / CMD keep them (pmf_cur_csr.h): indptr [lines_p + 1] int64 with the pad lines empty,
// indices [nnz] int32 strictly ascending within a line, vals [nnz] float32.  A stored zero is a zero.
//
// k_greedy_csr_pass<CPL>  one round of the wide case: the lines of the image whose lines are the candidate columns (the image of V^T,
//                         or of V for the selection on the transposed view) against the staged operand Op [Rp][128] float32 of
//                         k_greedy_step (B' in columns 0 .. c-1, Q behind it).  256 threads; a workgroup takes lines_per_wg
//                         consecutive lines, wave w of it lines w, w + 4, ...  The wave loads 64 entries of its line in one coalesced
//                         read and hands them round by v_readlane, four at a time; for an entry (r, v) lane l reads Op[r][l] (and
//                         Op[r][l + 64]: CPL = 2, launched once c + i > 64), one contiguous 256-byte read per entry and half, the four
//                         rows in flight together.  v * Op is exact in float64 (24 x 24 bits); entry e of the line is added to
//                         accumulator e mod 4 in line order, the line's sum is (a0 + a1) + (a2 + a3).  The squares of the sums of
//                         lanes < c make the numerator, the others |Q^T v|^2, both by the xor tree 32, 16, ..., 1.  The score against
//                         the float64 norm carries the residual guard of k_greedy_pass's epilogue; a chosen line scores -1, an empty
//                         line has norm 0 and scores 0, pad lines are not swept.  A wave keeps its best score and, its lines
//                         ascending, the lowest line attaining it; the workgroup writes one partial (sivm_wg_best), which
//                         k_greedy_step_csr reduces as k_greedy_step does.  No atomics, no LDS beyond the reduce, no private segment;
//                         the order of every sum follows from the line's length alone: two runs give the same bits.
// k_greedy_csr_gather     W [mp][KP] float32 (zeroed by the host in stream order): the stored entries of column sel[j], a line of
//                         the image of V^T, into column j; one workgroup per j.
// k_greedy_csr_pinv_t     B [mp][64] float64 = (P W^T)^T, P [k][k] the pseudo-inverse of W^T W: the operand of H^T = V^T pinv(W)^T
//                         on k_csr_proj_f64; rows >= m and columns >= k zero.
// k_greedy_csr_widen      Wd [mp][64] float64 = W [mp][KP] float32 (columns >= k zero): the error's copy of W.
// k_greedy_csr_ht         HT [np][64] float64 <-> H [KP][np] float32, either way (to_h: rounded once).
#pragma once
#include "pmf_greedy.h"

constexpr int PMF_GCSR_LD = 64;             // leading dimension of the float64 side arrays: PMF_GREEDY_MAX_BASES, one panel of k_csr_proj_f64
constexpr int PMF_GCSR_MIN_LINES = 64;      // lines a workgroup of k_greedy_csr_pass takes at least (16 per wave)

struct GreedyCsrPassArgs {
  const int64_t* indptr;       // [lines + 1 or more] the image whose lines are the candidates
  const int32_t* indices;      // row ids of the operand, < its row count (the host checks: csr_check)
  const float* vals;
  const float* Op;             // [rows padded][PMF_GREEDY_OPW]
  const double* nrm2;          // [lines padded] |v_j|^2
  const unsigned char* taken;  // [lines padded]
  double* pscore;              // [wgs]
  int* pidx;
  int lines, lines_per_wg;     // candidates; lines_per_wg a multiple of 4
  int c;                       // columns of B'
};

template <int CPL>
__global__ __launch_bounds__(256) void k_greedy_csr_pass(const GreedyCsrPassArgs a) {
  static_assert(CPL == 1 || CPL == 2, "the operand is one or two 64-column halves across");
  __shared__ double sb[4];
  __shared__ int ib[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l_begin = (int)blockIdx.x * a.lines_per_wg;
  const int l_end = min(l_begin + a.lines_per_wg, a.lines);
  const float* Opl = a.Op + lane;
  double best = -2.0;
  int bidx = 0x7fffffff;
#pragma unroll 1
  for (int line = l_begin + wv; line < l_end; line += 4) {   // (uniform over the wave)
    const int64_t hi = a.indptr[line + 1];
    double acc[CPL][4];
#pragma unroll
    for (int h = 0; h < CPL; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[h][e] = 0.0;
    for (int64_t f0 = a.indptr[line]; f0 < hi; f0 += 64) {
      const int cnt = (int)(hi - f0 < 64 ? hi - f0 : 64);
      const int my_i = lane < cnt ? a.indices[f0 + lane] : 0;
      const int my_v = lane < cnt ? __float_as_int(a.vals[f0 + lane]) : 0;
      int s = 0;
      for (; s + 4 <= cnt; s += 4) {
        int ri[4];
        double v[4];
        float b[CPL][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ri[e] = __builtin_amdgcn_readlane(my_i, s + e);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int h = 0; h < CPL; ++h) b[h][e] = Opl[(int64_t)ri[e] * PMF_GREEDY_OPW + 64 * h];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + e));
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int h = 0; h < CPL; ++h) acc[h][e] = fma(v[e], (double)b[h][e], acc[h][e]);
      }
      if (s < cnt) {                              // the last one to three entries of the line (s is a multiple of 4)
        const int r0 = __builtin_amdgcn_readlane(my_i, s);
        const int r1 = __builtin_amdgcn_readlane(my_i, s + 1 < cnt ? s + 1 : s), r2 = __builtin_amdgcn_readlane(my_i, s + 2 < cnt ? s + 2 : s);
        const double v0 = (double)__int_as_float(__builtin_amdgcn_readlane(my_v, s));
        const double v1 = s + 1 < cnt ? (double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 1)) : 0.0;
        const double v2 = s + 2 < cnt ? (double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 2)) : 0.0;
#pragma unroll
        for (int h = 0; h < CPL; ++h) {
          const float b0 = Opl[(int64_t)r0 * PMF_GREEDY_OPW + 64 * h], b1 = Opl[(int64_t)r1 * PMF_GREEDY_OPW + 64 * h];
          const float b2 = Opl[(int64_t)r2 * PMF_GREEDY_OPW + 64 * h];
          acc[h][0] = fma(v0, (double)b0, acc[h][0]);
          if (s + 1 < cnt) acc[h][1] = fma(v1, (double)b1, acc[h][1]);
          if (s + 2 < cnt) acc[h][2] = fma(v2, (double)b2, acc[h][2]);
        }
      }
    }
    // operand column `lane` belongs to B' for lane < c and to Q otherwise; column lane + 64 is always Q's (c <= 64)
    const double g0 = (acc[0][0] + acc[0][1]) + (acc[0][2] + acc[0][3]);
    double num = lane < a.c ? g0 * g0 : 0.0;
    double qs = lane < a.c ? 0.0 : g0 * g0;
    if constexpr (CPL == 2) {
      const double g1 = (acc[1][0] + acc[1][1]) + (acc[1][2] + acc[1][3]);
      qs = fma(g1, g1, qs);
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
      num += __shfl_xor(num, x);
      qs += __shfl_xor(qs, x);
    }
    // The residual guard of k_greedy_pass's epilogue, restated: that kernel's text stays as it is, so that its code object does.
    const double v2 = a.nrm2[line];
    const double den = v2 - qs;
    double sc = (den > 0.0 && den > PMF_GREEDY_TAU32 * v2) ? num / den : 0.0;
    if (a.taken[line]) sc = -1.0;
    if (sc > best) { best = sc; bidx = line; }    // lines ascend per wave: a strict > keeps the lowest index
  }
  sivm_wg_best(best, bidx, sb, ib);
  if (threadIdx.x == 0) { a.pscore[blockIdx.x] = best; a.pidx[blockIdx.x] = bidx; }
}

// grid = k workgroups; sel[j] in [0, n) (k_greedy_step_csr and k_greedy_gram write nothing else)
__global__ __launch_bounds__(256) void k_greedy_csr_gather(const int64_t* __restrict__ tindptr, const int32_t* __restrict__ tindices,
                                                           const float* __restrict__ tvals, const int* __restrict__ sel, int KP,
                                                           float* __restrict__ W) {
  const int j = (int)blockIdx.x, col = sel[j];
  const int64_t hi = tindptr[col + 1];
  for (int64_t e = tindptr[col] + threadIdx.x; e < hi; e += 256) W[(int64_t)tindices[e] * KP + j] = tvals[e];
}

__global__ __launch_bounds__(256) void k_greedy_csr_pinv_t(const float* __restrict__ W, const double* __restrict__ P, int64_t m, int k, int KP,
                                                           int64_t elems, double* __restrict__ B) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  const int64_t r = e / PMF_GCSR_LD;
  const int j = (int)(e % PMF_GCSR_LD);
  double s = 0.0;
  if (r < m && j < k)
    for (int q = 0; q < k; ++q) s = fma(P[(int64_t)j * k + q], (double)W[r * KP + q], s);
  B[e] = s;
}

__global__ __launch_bounds__(256) void k_greedy_csr_widen(const float* __restrict__ W, int KP, int k, int64_t elems, double* __restrict__ Wd) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  const int64_t r = e / PMF_GCSR_LD;
  const int j = (int)(e % PMF_GCSR_LD);
  Wd[e] = j < k ? (double)W[r * KP + j] : 0.0;
}

// elems = np * 64; to_h: H[j][col] = (float) HT[col][j] for j < k; otherwise HT[col][j] = H[j][col] (columns >= k zero)
__global__ __launch_bounds__(256) void k_greedy_csr_ht(float* __restrict__ H, int np, int k, int64_t elems, double* __restrict__ HT, int to_h) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  const int64_t col = e / PMF_GCSR_LD;
  const int j = (int)(e % PMF_GCSR_LD);
  if (to_h) {
    if (j < k) H[(int64_t)j * np + col] = (float)HT[e];
  } else {
    HT[e] = j < k ? (double)H[(int64_t)j * np + col] : 0.0;
  }
}
