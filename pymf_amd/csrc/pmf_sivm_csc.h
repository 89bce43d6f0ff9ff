// pmf_sivm_csc.h -- SIVM and LAESA on CSC data (sivm.py:110-120, dist.py:37-42: the reference's sparse branch): the selection pass,
// the gather of W and the W^T V block of the H step over stored entries only.  No dense V exists on such a context.
//
// CSC arrays: indptr [np + 1] int64 (columns >= n are empty), indices [nnz] int32 (row ids, ascending within a column, no
// duplicates: checked on the host before the upload), vals [nnz] float32.
//
// k_sivm_csc_pass<METRIC, RULE, TEAM> keeps the contract of the sweep of pmf_colsweep.h -- prologue (colsweep_pick), partials and
// argmax chain (colsweep_finish), tie, NaN and pad rules (sivm_better; only c < n is offered), the panel partition -- and
// replaces colsweep_stage_x and colsweep_sums:
//   x    the measured column is scattered dense into the m floats of dynamic LDS: zeroed, then column idx written over it
//        (idx = -1: the origin, zeros).  |x|^2 and |x|_1 once per workgroup from the stored entries of column idx: thread t sums
//        entries t, t + 256, ... in order, then the xor tree over the 64 lanes, then the four waves in order -- every workgroup
//        the same bits.
//   sums a team of TEAM adjacent lanes owns one column; lane t takes entries t, t + TEAM, ... (a wave reads one contiguous run of
//        vals and indices: its teams own adjacent columns), one fp32 running sum per lane, the team's sums combined by the xor
//        tree TEAM / 2, ..., 1.  Over the stored entries (v, r) of the column:
//          l2      |x|^2 + sum [(v - x_r)^2 - x_r^2], clamped at 0 before sqrtf
//          l1      |x|_1 + sum [|v - x_r| - |x_r|], clamped at 0
//          cosine  sum v x_r and sum v^2, then colsweep_dist<COSINE>'s formula 1 - v.x / (|v| |x| + 1e-9)
//        c == idx: the l2 and l1 distances are exactly 0, as the difference form of the dense pass gives (the sums above leave
//        rounding noise there).  An empty column is the origin.
//   RULE 0: SIVM's recurrence (sivm_recur) on dij, dsum, dsq; RULE 1: LAESA's running minimum on st0 (k_laesa_pass).  States and
//        scores float64.
// The summation order depends on TEAM and on nothing else: two runs with the same TEAM give the same bits.  No float atomics.
// k_sivm_csc_gather  W[:, j] = column select[j] densified (-1: the last column, as k_sivm_gather reads it) into a zeroed W.
// k_csc_wtv<NT>      PS[j][c] = sum over the stored entries (v, r) of column c of v W[r][j], float64 fma in entry order, rounded to
//                    float32 once (the right-hand sides then carry one rounding, as the dense H step's oracle assumes): a team of
//                    KP = 16 NT lanes per column, lane j the base j (a row of W is one contiguous read, W stays in L2); a
//                    workgroup owns one 64-column panel and writes it through LDS so that the stores run along the rows of PS.
#pragma once
#include "pmf_sivm.h"

enum { PMF_CSC_RULE_SIVM = 0, PMF_CSC_RULE_LAESA = 1 };

struct SivmCscArgs : ColsweepPickArgs {   // (V stays null; np is the stride of the state arrays)
  const int64_t* indptr;
  const int32_t* indices;
  const float* vals;
  double* st0;             // [np] SIVM: d_i_times_d_j; LAESA: dmin
  double* st1;             // [np] SIVM: d_sum
  double* st2;             // [np] SIVM: d_square
  int plain;               // score = dist, state untouched
  int first;               // LAESA: the first recurrence round (dmin = d)
  int l;                   // SIVM: step of the recurrence (sivm.py:181)
};

// the sum of s over the 64 lanes in fp32, a fixed order, the same bits in every lane
__device__ __forceinline__ float csc_wave_sum(float s) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) s += __shfl_xor(s, x);
  return s;
}

// x = column idx scattered into xs[0 .. m) (idx < 0: zeros); *xx = |x|^2, *x1 = |x|_1
__device__ __forceinline__ void csc_stage_x(const SivmCscArgs& a, int idx, float* xs, float* wsum, float* xx, float* x1) {
  for (int r = threadIdx.x; r < a.m; r += 256) xs[r] = 0.f;
  __syncthreads();
  float sq = 0.f, ab = 0.f;
  if (idx >= 0) {
    const int64_t hi = a.indptr[idx + 1];
    for (int64_t e = a.indptr[idx] + threadIdx.x; e < hi; e += 256) {
      const float v = a.vals[e];
      xs[a.indices[e]] = v;                        // (row ids < m and distinct within a column: checked before the upload)
      sq = fmaf(v, v, sq);
      ab += fabsf(v);
    }
  }
  sq = csc_wave_sum(sq);
  ab = csc_wave_sum(ab);
  if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = sq; wsum[4 + (threadIdx.x >> 6)] = ab; }
  __syncthreads();
  *xx = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  *x1 = ((wsum[4] + wsum[5]) + wsum[6]) + wsum[7];
}

template <int METRIC, int RULE, int TEAM>
__global__ __launch_bounds__(256) void k_sivm_csc_pass(const SivmCscArgs a) {
  static_assert(TEAM == 4 || TEAM == 16 || TEAM == 64, "a team is a power of two within one wave");
  extern __shared__ float xs[];                 // [m]
  __shared__ double sb[4];
  __shared__ int ib[4];
  __shared__ float wsum[8];
  double a_log;
  const int idx = colsweep_pick(a, sb, ib, &a_log);
  if (RULE == PMF_CSC_RULE_SIVM && !a.take_maxd && !a.plain) a_log = a.scal[1];
  const double hl = 0.5 * (double)a.l;
  float xx, x1;
  csc_stage_x(a, idx, xs, wsum, &xx, &x1);

  constexpr int CPT = 256 / TEAM;               // columns of one trip of the workgroup
  const int t = threadIdx.x & (TEAM - 1), g = threadIdx.x / TEAM;
  const int c_begin = blockIdx.x * a.panels_per_wg * 64;
  const int c_end = min(min((blockIdx.x + 1) * a.panels_per_wg, a.npanels) * 64, a.n);
  double bs = -INFINITY;
  int bidx = 0x7fffffff;
  for (int cb = c_begin; cb < c_end; cb += CPT) {   // (uniform trip count: the shuffles below are executed by every lane)
    const int c = cb + g;
    int64_t lo = 0, hi = 0;
    if (c < c_end) { lo = a.indptr[c]; hi = a.indptr[c + 1]; }
    float s = 0.f, nn = 0.f;
    for (int64_t e = lo + t; e < hi; e += TEAM) {
      const float v = a.vals[e];
      const float x = xs[a.indices[e]];
      if (METRIC == PMF_SIVM_L2) {
        const float d = v - x;
        s += d * d - x * x;
      } else if (METRIC == PMF_SIVM_L1) {
        s += fabsf(v - x) - fabsf(x);
      } else {
        s = fmaf(v, x, s);
        nn = fmaf(v, v, nn);
      }
    }
#pragma unroll
    for (int x = TEAM / 2; x >= 1; x >>= 1) {
      s += __shfl_xor(s, x);
      if (METRIC == PMF_SIVM_COSINE) nn += __shfl_xor(nn, x);
    }
    if (t != 0 || c >= c_end) continue;
    float dist;
    if (METRIC == PMF_SIVM_L2) dist = c == idx ? 0.f : sqrtf(fmaxf(xx + s, 0.f));
    else if (METRIC == PMF_SIVM_L1) dist = c == idx ? 0.f : fmaxf(x1 + s, 0.f);
    else dist = 1.f - s / (sqrtf(nn) * sqrtf(xx) + 1e-9f);   // colsweep_dist<PMF_SIVM_COSINE>
    double d = (double)dist;
    if (!a.plain) {
      if (RULE == PMF_CSC_RULE_SIVM) {
        d = sivm_recur(d, a_log, hl, a.st0, a.st1, a.st2, c);
      } else {
        if (!a.first) {
          const double old = a.st0[c];
          d = d < old ? d : old;                   // (a NaN d keeps the old minimum)
        }
        a.st0[c] = d;
      }
    }
    sivm_better(bs, bidx, d, c);
  }
  colsweep_finish(a, bs, bidx, sb, ib);
}

// W [mp][KP], zeroed by the caller: workgroup j scatters column select[j] (-1: the last data column) into W[:, j]
__global__ __launch_bounds__(256) void k_sivm_csc_gather(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                         const float* __restrict__ vals, int n, int KP, const int* __restrict__ select,
                                                         float* __restrict__ W) {
  const int j = blockIdx.x;
  int s = select[j];
  if (s < 0) s += n;
  s = min(max(s, 0), n - 1);
  const int64_t hi = indptr[s + 1];
  for (int64_t e = indptr[s] + threadIdx.x; e < hi; e += 256) W[(int64_t)indices[e] * KP + j] = vals[e];
}

// the W^T V block of dPS [KP][ldp] for the 64-column panel blockIdx.x; columns >= n (empty) and bases >= k (zero columns of W): 0
template <int NT>
__global__ __launch_bounds__(256) void k_csc_wtv(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                 const float* __restrict__ vals, const float* __restrict__ W, float* __restrict__ PS,
                                                 int64_t ldp) {
  constexpr int KP = 16 * NT, CPT = 256 / KP;
  __shared__ float tile[KP][65];
  const int j = threadIdx.x % KP, g = threadIdx.x / KP;
  const int64_t c0 = (int64_t)blockIdx.x * 64;
  for (int q = g; q < 64; q += CPT) {
    const int64_t hi = indptr[c0 + q + 1];
    double acc = 0.0;                              // (float64, rounded once: fp32 running sums over ~125 entries miss the H bound at cond(W^T W) ~ 1e4)
    for (int64_t e = indptr[c0 + q]; e < hi; ++e) acc = fma((double)vals[e], (double)W[(int64_t)indices[e] * KP + j], acc);
    tile[j][q] = (float)acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < KP * 64; i += 256) PS[(int64_t)(i >> 6) * ldp + c0 + (i & 63)] = tile[i >> 6][i & 63];
}
