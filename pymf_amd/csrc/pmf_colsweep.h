// pmf_colsweep.h -- the sweep over the resident V [mp][np] that every column-selection pass of a SIVM context runs:
// k_sivm_pass (pmf_sivm.h), k_laesa_pass and k_gmap_pass (pmf_colsel.h), k_sgreedy_pass (pmf_sgreedy.h).
//
// A launch measures every column against ONE column x = V[:, idx], updates a pointwise state and takes an argmax.  A workgroup
// owns a contiguous range of 64-column panels (colsweep_quads), a lane 4 adjacent columns with one 16-byte read per row; x is
// staged in dynamic LDS (m floats, idx = -1: the origin, zeros) and read as a broadcast (every lane the same word: no bank
// conflict); the rows are walked four at a time with four independent fp32 partial sums per column and tails of 1, 2 and 3 rows
// (colsweep_sums).  Argmax without a host round trip and without float atomics: every workgroup writes (best score, lowest
// column attaining it) into a partials array (colsweep_finish); the NEXT launch reduces the <= PMF_CL_MAX_WGS partials in its
// prologue -- every workgroup the same way -- and works on that idx, workgroup 0 appends it to select[] (colsweep_pick);
// k_sivm_close does the last reduce.  By construction: the lowest index wins ties and a NaN score never wins (sivm_better), pad
// columns (c >= n) never win (the kernels offer only c < n), an index outside [0, n) is never gathered (sivm_reduce_partials),
// two runs give the same bits.  What a kernel adds is the score and the state update of one quad of columns.
#pragma once
#include "pmf_dev.h"

enum { PMF_SIVM_L2 = 0, PMF_SIVM_L1 = 1, PMF_SIVM_COSINE = 2 };         // the metrics, and what colsweep_sums accumulates for them;
enum { PMF_COLSEL_DOT = 3, PMF_COLSEL_SQ = 4, PMF_COLSEL_SQSUM = 5 };   // its other modes

// what every pass takes: the matrix, the partition and the two partials arrays; by value, as the head of the kernel's argument
struct ColsweepArgs {
  const float* V;          // [mp][np]
  const double* pscore_in; // partials of the previous launch ...
  const int* pidx_in;
  double* pscore_out;      // ... and of this one, [wgs]
  int* pidx_out;
  int64_t np;
  int m, n;
  int npanels, panels_per_wg;
  int nprev;               // partials of the previous launch to reduce in the prologue (0: none)
};

// ... and the passes whose prologue is colsweep_pick
struct ColsweepPickArgs : ColsweepArgs {
  int* select;             // [k]
  double* scal;            // [0] maxd, [1] a = log(maxd)
  int use_fixed;           // idx = fixed_idx (the first fastmap pass: column 0; 'origin': -1) instead of the prologue's argmax
  int fixed_idx;
  int sel_pos;             // >= 0: workgroup 0 writes select[sel_pos] = idx
  int take_maxd;           // the best score of the previous (plain) launch is maxd: workgroup 0 stores it and its logarithm
};

// (score, index): a greater score wins, then the lower index
__device__ __forceinline__ void sivm_better(double& s, int& i, double os, int oi) {
  if (os > s || (os == s && oi < i)) { s = os; i = oi; }
}

// the workgroup's best of (s, i) over its 256 threads, in thread 0 (and in sb[0], ib[0])
__device__ __forceinline__ void sivm_wg_best(double& s, int& i, double* sb, int* ib) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const double os = __shfl_xor(s, x);
    const int oi = __shfl_xor(i, x);
    sivm_better(s, i, os, oi);
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sb[wave] = s; ib[wave] = i; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) sivm_better(s, i, sb[w], ib[w]);
    sb[0] = s; ib[0] = i;
  }
  __syncthreads();
}

// the argmax over the previous launch's partials (every workgroup alike); n: an index outside [0, n) -- no finite score at
// all -- becomes 0, so that nothing is ever gathered from outside V
__device__ __forceinline__ void sivm_reduce_partials(const double* ps, const int* pi, int count, int n, double* sb, int* ib,
                                                     double* best, int* idx) {
  double s = -INFINITY;
  int i = 0x7fffffff;
  for (int q = threadIdx.x; q < count; q += 256) sivm_better(s, i, ps[q], pi[q]);
  sivm_wg_best(s, i, sb, ib);
  *best = sb[0];
  *idx = ((unsigned)ib[0] < (unsigned)n) ? ib[0] : 0;
}

// prologue: the column this pass measures against, recorded by workgroup 0; *log_maxd: log(maxd) behind the last plain pass
// (take_maxd), otherwise 0
__device__ __forceinline__ int colsweep_pick(const ColsweepPickArgs& a, double* sb, int* ib, double* log_maxd) {
  int idx = a.fixed_idx;
  *log_maxd = 0.0;
  const bool rec = blockIdx.x == 0 && threadIdx.x == 0;
  if (a.nprev > 0) {
    double best;
    int bi;
    sivm_reduce_partials(a.pscore_in, a.pidx_in, a.nprev, a.n, sb, ib, &best, &bi);
    if (!a.use_fixed) idx = bi;
    if (a.take_maxd) {
      *log_maxd = log(best);
      if (rec) { a.scal[0] = best; a.scal[1] = *log_maxd; }
    }
  }
  if (rec && a.sel_pos >= 0) a.select[a.sel_pos] = idx;
  return idx;
}

// x = V[:, idx] into LDS (idx < 0: the origin)
__device__ __forceinline__ void colsweep_stage_x(const ColsweepArgs& a, int idx, float* xs) {
  const float* xcol = a.V + (idx >= 0 ? idx : 0);
  for (int r = threadIdx.x; r < a.m; r += 256) xs[r] = idx >= 0 ? xcol[(int64_t)r * a.np] : 0.f;
  __syncthreads();
}

// the fp32 sums of the lane's 4 columns c .. c + 3 down the m rows, four independent partial sums each:
//   L2 s = sum (v - x)^2;  L1 s = sum |v - x|;  COSINE s = v . x, nn = |v|^2, xx = |x|^2;  DOT s = v . x;
//   SQ nn = |v|^2;  SQSUM nn = |v|^2, s = sum v  (SQ, SQSUM: xs is not read)
template <int MODE>
__device__ __forceinline__ void colsweep_sums(const ColsweepArgs& a, int c, const float* xs, f32x4& st, f32x4& nt, float& xt) {
  const float* vp = a.V + c;
  const int64_t np = a.np;
  const int m = a.m;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
  f32x4 n0 = s0, n1 = s0, n2 = s0, n3 = s0;
  f32x4 xp = s0;                                    // the four partial sums of |x|^2: one vector, so that they pair with xs[r .. r + 3]
  constexpr bool kNeedsX = MODE != PMF_COLSEL_SQ && MODE != PMF_COLSEL_SQSUM;
  auto step = [&](const f32x4 v, const int r, f32x4& s, f32x4& nn, const int j) {
    const float x = kNeedsX ? xs[r] : 0.f;
    if (MODE == PMF_SIVM_L2) {
      const f32x4 d = v - x;
      s += d * d;
    } else if (MODE == PMF_SIVM_L1) {
      const f32x4 d = v - x;
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += fabsf(d[e]);
    } else if (MODE == PMF_SIVM_COSINE) {
      s += v * x;
      nn += v * v;
      xp[j] = fmaf(x, x, xp[j]);
    } else if (MODE == PMF_COLSEL_DOT) {
      s += v * x;
    } else if (MODE == PMF_COLSEL_SQ) {
      nn += v * v;
    } else {
      nn += v * v;
      s += v;
    }
  };
  int r = 0;
  for (; r + 4 <= m; r += 4) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 0) * np);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 1) * np);
    const f32x4 v2 = *reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 2) * np);
    const f32x4 v3 = *reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 3) * np);
    step(v0, r + 0, s0, n0, 0);
    step(v1, r + 1, s1, n1, 1);
    step(v2, r + 2, s2, n2, 2);
    step(v3, r + 3, s3, n3, 3);
  }
  if (r < m) step(*reinterpret_cast<const f32x4*>(vp + (int64_t)r * np), r, s0, n0, 0);
  if (r + 1 < m) step(*reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 1) * np), r + 1, s1, n1, 1);
  if (r + 2 < m) step(*reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 2) * np), r + 2, s2, n2, 2);
  st = (s0 + s1) + (s2 + s3);
  nt = (n0 + n1) + (n2 + n3);
  xt = (xp[0] + xp[1]) + (xp[2] + xp[3]);
}

// the distance to x of the lane's 4 columns from colsweep_sums<METRIC>'s sums, as dist.py:57-63 forms it (from the difference)
template <int METRIC>
__device__ __forceinline__ f32x4 colsweep_dist(const f32x4 st, const f32x4 nt, const float xx) {
  f32x4 dist = st;                                  // l1
  if (METRIC == PMF_SIVM_L2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) dist[e] = sqrtf(st[e]);
  } else if (METRIC == PMF_SIVM_COSINE) {
    const float xn = sqrtf(xx);
#pragma unroll
    for (int e = 0; e < 4; ++e) dist[e] = 1.f - st[e] / (sqrtf(nt[e]) * xn + 1e-9f);
  }
  return dist;
}

// this workgroup's panel range: its first column and its number of quads (>= 16: a workgroup owns at least one panel)
__device__ __forceinline__ void colsweep_quad_range(const ColsweepArgs& a, int* c_begin, int* nquads) {
  *c_begin = blockIdx.x * a.panels_per_wg * 64;
  const int c_end = min((blockIdx.x + 1) * a.panels_per_wg, a.npanels) * 64;
  *nquads = (c_end - *c_begin) / 4;
}

// f(c) for the first column c of every quad of this workgroup's panel range (f: a lambda, inlined)
template <class F>
__device__ __forceinline__ void colsweep_quads(const ColsweepArgs& a, F f) {
  int c_begin, nquads;
  colsweep_quad_range(a, &c_begin, &nquads);
  for (int q = threadIdx.x; q < nquads; q += 256) f(c_begin + 4 * q);
}

// the same with uniform trips, for a body that holds barriers: f(c, live) runs in every lane of the workgroup the same number
// of times; a lane beyond the last quad gets the last quad again with live = false (it may read, and must offer and write nothing)
template <class F>
__device__ __forceinline__ void colsweep_quads_uniform(const ColsweepArgs& a, F f) {
  int c_begin, nquads;
  colsweep_quad_range(a, &c_begin, &nquads);
  for (int qb = 0; qb < nquads; qb += 256) {
    const int q = qb + (int)threadIdx.x;
    f(c_begin + 4 * min(q, nquads - 1), q < nquads);
  }
}

// epilogue: the workgroup's (best score, lowest column attaining it) into this launch's partials
__device__ __forceinline__ void colsweep_finish(const ColsweepArgs& a, double bs, int bidx, double* sb, int* ib) {
  sivm_wg_best(bs, bidx, sb, ib);
  if (threadIdx.x == 0) { a.pscore_out[blockIdx.x] = bs; a.pidx_out[blockIdx.x] = bidx; }
}
