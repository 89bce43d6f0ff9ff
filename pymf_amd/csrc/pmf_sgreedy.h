// pmf_sgreedy.h -- SIVM_SGREEDY (pymf/sivm_sgreedy.py:96-133): greedy selection by the exact simplex volume.  Runs on a SIVM
// context (pmf_set_option "sivm_sgreedy").
//
// The reference scores column i in round t (t columns S selected so far) by the Cayley-Menger volume of S + {i}
//   V[i] = sqrt(|f1(t) det(CM(S + {i}))|),   f1(j) = (-1)^(j+1) / (2^j (j!)^2)                          (vol.py:24-34)
// with one determinant per column.  The candidate enters CM as one bordered row and column with a zero corner, so
//   det(CM(S + {i})) = det(CM_S) (-b_i^T M b_i),   M = inv(CM_S),   b_i = [1, d^2(i, s_1), ..., d^2(i, s_t)]
// and M, det(CM_S) are shared by all columns: at most 64 x 64, float64, from one workgroup (k_sgreedy_step); the per-column
// work is t + 1 squared l2 distances and one quadratic form (k_sgreedy_pass).  S is kept in selection order through the rounds:
// the determinant does not depend on the order; k_sgreedy_order puts `select` into the reference's order behind the last round.
//
// k_sgreedy_pass  one launch per round on the sweep of pmf_colsweep.h (x = the newest selected column in dynamic LDS, behind it
//   M).  The fp32 squared l2 distance to x is colsweep_sums' difference sum (what k_laesa_pass<l2> takes the root of); it
//   becomes row t - 1 of the float32 table d2 [64][np]; rows 0 .. t - 1 are read back and b^T M b is formed in float64 on the
//   vector unit in 8 x 8 blocks of M: a lane holds two blocks of b (8 entries x 4 columns each, compile-time indexed) and walks
//   the lower block triangle, the off-diagonal blocks counting twice.  score = sqrt(|scale_t form|), scale_t = |f1(t) det(CM_S)|.
// k_sgreedy_step  one workgroup between two passes: the argmax of the previous launch is s_t (its score the volume of the round
//   before: _v); CM_S is gathered from the table -- d^2(s_i, s_j) = d2[i - 1][s_j], i < j, the very fp32 values the candidates
//   see, so a candidate equal to a selected column scores rounding-level zero -- and inverted in place in LDS by Gauss-Jordan
//   with row pivoting (CM_S is indefinite); det from the pivots, folded with f1 factor by factor so that neither over- nor
//   underflows on its own.  A singular CM_S (S affinely dependent: num_bases > rows + 1) gives a non-finite M; such scores never
//   win (sivm_better), the prologue's index stays inside [0, n).
#pragma once
#include "pmf_colsweep.h"

constexpr int PMF_SGREEDY_MAX_T = 64;    // order of CM_S at the last round: 63 selected columns and the border
constexpr int PMF_SGREEDY_BLK = 8;       // block edge of the quadratic form

struct SgreedyArgs : ColsweepArgs {
  float* d2;               // [64][np] squared l2 distances: row r to the (r + 1)-th selected column
  double* M;               // [64][64] inv(CM_S), zero outside its (t + 1) x (t + 1)
  double* sc;              // [0] scale_t
  double* vol;             // [64] the volumes of the rounds (_v)
  int* select;             // [k] in selection order
  int t;                   // columns selected so far (this round finds the (t + 1)-th)
  int origin;              // init = 'origin': select[0] = -1, the first vertex is the LAST data column (sivm_sgreedy.py:99,109)
};

// the column the round measures against: the argmax of the previous launch, or under 'origin' in round 1 the last data column
__device__ __forceinline__ int sgreedy_newest(const SgreedyArgs& a, double* sb, int* ib, double* best) {
  int idx;
  sivm_reduce_partials(a.pscore_in, a.pidx_in, a.nprev, a.n, sb, ib, best, &idx);
  return (a.origin && a.t == 1) ? a.n - 1 : idx;
}

__global__ __launch_bounds__(256) void k_sgreedy_step(const SgreedyArgs a) {
  constexpr int LD = PMF_SGREEDY_MAX_T + 1;     // (odd stride: a column walk touches every bank)
  __shared__ double A[PMF_SGREEDY_MAX_T * LD];
  __shared__ double frow[PMF_SGREEDY_MAX_T], fcol[PMF_SGREEDY_MAX_T];
  __shared__ int sel[PMF_SGREEDY_MAX_T], perm[PMF_SGREEDY_MAX_T];
  __shared__ double sb[4];
  __shared__ int ib[4];
  __shared__ double s_piv;
  __shared__ int s_prow;
  const int tid = threadIdx.x;
  const int t = a.t, T = t + 1;

  double best;
  const int idx = sgreedy_newest(a, sb, ib, &best);
  if (tid == 0) {
    a.select[t - 1] = (a.origin && t == 1) ? -1 : idx;
    if (t >= 2) a.vol[t - 2] = best;            // the previous pass's winning score: the volume of its round
  }
  if (tid < t) {
    const int s = tid == t - 1 ? idx : a.select[tid];
    sel[tid] = s < 0 ? a.n - 1 : s;
  }
  __syncthreads();

  // ---- CM_S: index 0 the border of ones, index j the j-th selected column ---------------------------------------------------
  for (int e = tid; e < T * T; e += 256) {
    const int i = e / T, j = e % T;
    double v;
    if (i == j) v = 0.0;
    else if (i == 0 || j == 0) v = 1.0;
    else v = (double)a.d2[(int64_t)(min(i, j) - 1) * a.np + sel[max(i, j) - 1]];
    A[i * LD + j] = v;
  }
  __syncthreads();

  // ---- inverse in place: Gauss-Jordan, row pivoting, the swaps undone on the columns at the end ------------------------------
  double scale = 1.0;                            // (thread 0) |piv_0| prod_j |piv_j| / (2 j^2) = |f1(t) det(CM_S)|
  for (int p = 0; p < T; ++p) {
    if (tid < 64) {                              // the pivot: the largest modulus in column p from row p down, the lowest row on a tie
      double v = (tid >= p && tid < T) ? fabs(A[tid * LD + p]) : -1.0;
      int r = tid;
#pragma unroll
      for (int x = 1; x < 64; x <<= 1) {
        const double ov = __shfl_xor(v, x);
        const int orow = __shfl_xor(r, x);
        if (ov > v || (ov == v && orow < r)) { v = ov; r = orow; }
      }
      if (tid == 0) { s_prow = (v >= 0.0) ? r : p; perm[p] = s_prow; }   // (a column of NaNs: no swap)
    }
    __syncthreads();
    const int pr = s_prow;
    if (pr != p && tid < T) {
      const double u = A[p * LD + tid];
      A[p * LD + tid] = A[pr * LD + tid];
      A[pr * LD + tid] = u;
    }
    __syncthreads();
    if (tid == 0) {
      const double piv = A[p * LD + p];
      s_piv = piv;
      scale *= p == 0 ? fabs(piv) : fabs(piv) / (2.0 * (double)p * (double)p);
    }
    __syncthreads();
    if (tid < T) {
      const double piv = s_piv;
      frow[tid] = (tid == p ? 1.0 : A[p * LD + tid]) / piv;
      fcol[tid] = tid == p ? 0.0 : A[tid * LD + p];
    }
    __syncthreads();
    for (int e = tid; e < T * T; e += 256) {
      const int i = e / T, j = e % T;
      if (i == p) A[e / T * LD + j] = frow[j];
      else A[i * LD + j] = (j == p ? 0.0 : A[i * LD + j]) - fcol[i] * frow[j];
    }
    __syncthreads();
  }
  for (int p = T - 1; p >= 0; --p) {
    const int pr = perm[p];
    if (pr != p && tid < T) {
      const double u = A[tid * LD + p];
      A[tid * LD + p] = A[tid * LD + pr];
      A[tid * LD + pr] = u;
    }
    __syncthreads();
  }

  for (int e = tid; e < PMF_SGREEDY_MAX_T * PMF_SGREEDY_MAX_T; e += 256) {
    const int i = e / PMF_SGREEDY_MAX_T, j = e % PMF_SGREEDY_MAX_T;
    a.M[e] = (i < T && j < T) ? A[i * LD + j] : 0.0;
  }
  if (tid == 0) a.sc[0] = scale;
}

// select[] from selection order into the reference's: the first k - 1 picks ascending (it re-sorts them at the top of every round,
// sivm_sgreedy.py:108), the last pick behind them; -1 ('origin') stays first.  Ranks, equal entries in their old order.
__global__ __launch_bounds__(64) void k_sgreedy_order(int* __restrict__ select, int k) {
  __shared__ int s[PMF_SGREEDY_MAX_T];
  const int j = threadIdx.x;
  if (j < k - 1) s[j] = select[j];
  __syncthreads();
  if (j >= k - 1) return;
  int rank = 0;
  for (int i = 0; i < k - 1; ++i) rank += (s[i] < s[j] || (s[i] == s[j] && i < j)) ? 1 : 0;
  select[rank] = s[j];
}

__global__ __launch_bounds__(256) void k_sgreedy_pass(const SgreedyArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [m rounded up to 4] x, then M [TP][TP] float64
  __shared__ double sb[4];
  __shared__ int ib[4];
  constexpr int B = PMF_SGREEDY_BLK;
  const int tid = threadIdx.x;
  const int t = a.t;
  const int nb = (t + 1 + B - 1) / B, TP = nb * B;
  double* Ms = reinterpret_cast<double*>(xs + ((a.m + 3) & ~3));

  double best;
  const int idx = sgreedy_newest(a, sb, ib, &best);
  const double scale = a.sc[0];

  for (int e = tid; e < TP * TP; e += 256) Ms[e] = a.M[(e / TP) * PMF_SGREEDY_MAX_T + e % TP];
  colsweep_stage_x(a, idx, xs);

  float* const newrow = a.d2 + (int64_t)(t - 1) * a.np;
  double bs = -INFINITY;
  int bidx = 0x7fffffff;
  colsweep_quads(a, [&](const int c) __attribute__((always_inline)) {
    f32x4 st, nt;
    float xx;
    colsweep_sums<PMF_SIVM_L2>(a, c, xs, st, nt, xx);
    *reinterpret_cast<f32x4*>(newrow + c) = st;

    // entry e of b for the lane's 4 columns: 1, then the table's rows 0 .. t - 1 (row t - 1 is st), zero behind them
    const float* tab = a.d2 + c;
    auto load_block = [&](const int blk, double (&b)[B][4]) {
#pragma unroll
      for (int i = 0; i < B; ++i) {
        const int e = blk * B + i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (e == 0) v = f32x4{1.f, 1.f, 1.f, 1.f};
        else if (e < t) v = *reinterpret_cast<const f32x4*>(tab + (int64_t)(e - 1) * a.np);
        else if (e == t) v = st;
#pragma unroll
        for (int x = 0; x < 4; ++x) b[i][x] = (double)v[x];
      }
    };
    double form[4] = {0.0, 0.0, 0.0, 0.0};
    for (int I = 0; I < nb; ++I) {
      double bI[B][4], bJ[B][4];
      double off[B][4], dia[B][4];
      load_block(I, bI);
#pragma unroll
      for (int i = 0; i < B; ++i)
#pragma unroll
        for (int x = 0; x < 4; ++x) off[i][x] = dia[i][x] = 0.0;
      for (int J = 0; J < I; ++J) {
        load_block(J, bJ);
        const double* mp = Ms + (I * B) * TP + J * B;
#pragma unroll
        for (int i = 0; i < B; ++i)
#pragma unroll
          for (int j = 0; j < B; ++j) {
            const double mij = mp[i * TP + j];
#pragma unroll
            for (int x = 0; x < 4; ++x) off[i][x] = fma(mij, bJ[j][x], off[i][x]);
          }
      }
      {
        const double* mp = Ms + (I * B) * TP + I * B;
#pragma unroll
        for (int i = 0; i < B; ++i)
#pragma unroll
          for (int j = 0; j < B; ++j) {
            const double mij = mp[i * TP + j];
#pragma unroll
            for (int x = 0; x < 4; ++x) dia[i][x] = fma(mij, bI[j][x], dia[i][x]);
          }
      }
#pragma unroll
      for (int i = 0; i < B; ++i)
#pragma unroll
        for (int x = 0; x < 4; ++x) form[x] = fma(bI[i][x], fma(2.0, off[i][x], dia[i][x]), form[x]);
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if (c + x < a.n) sivm_better(bs, bidx, sqrt(fabs(scale * form[x])), c + x);
  });
  colsweep_finish(a, bs, bidx, sb, ib);
}
