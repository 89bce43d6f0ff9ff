// pmf_colsel.h -- LAESA (pymf/laesa.py) and GMAP (pymf/gmap.py, robust_map = False): the two column selections that sweep the
// data like SIVM's update_w but carry a lighter recurrence.  They run on a SIVM context (pmf_set_option "sivm_rule").
//
// Work decomposition, argmax chain and buffers are k_sivm_pass's (pmf_sivm.h): a workgroup owns a contiguous range of 64-column
// panels, a lane 4 adjacent columns with one 16-byte read per row; x = V[:, idx] is staged in dynamic LDS (m floats) and read
// as a broadcast (every lane the same word: no bank conflict); the row loop is unrolled by four with four independent fp32
// partial sums and tails of 1, 2 and 3 rows; every workgroup writes (best score, lowest column attaining it) into a partials
// array that the NEXT launch reduces in its prologue (sivm_reduce_partials), k_sivm_close does the last reduce, k_sivm_gather
// writes W.  Pad columns (c >= n) never win, the lowest index wins ties, a NaN score never wins (sivm_better), no float atomics,
// no host read between rounds, two runs give the same bits.
//
// k_laesa_pass<METRIC>  (laesa.py:63-82)  the distance to x in fp32 as k_sivm_pass forms it (l2, l1, cosine; idx = -1: the
//   origin).  One float64 state array dmin[np].  Plain rounds (init_sivm, sivm.py:145-166: three for 'fastmap', one for
//   'origin') are SIVM's: score = dist, state untouched.  The first recurrence round writes dmin = d (the reference measures
//   against select[0] twice and takes the minimum of the two equal vectors: one pass here); later rounds
//   dmin = d < dmin ? d : dmin -- a NaN d keeps dmin, as np.where does; score = dmin.
// k_gmap_pass<METHOD>   (gmap.py:119-165) two float64 state arrays norm[np], iterval[np].  Round 0 has no x: the fp32 sum of
//   squares of every column (and its fp32 sum, 'nmf'), norm = sqrt(double(sum)), iterval = norm ('pca', 'aa') or
//   1 - colsum / (sqrt(m) norm) ('nmf'), argmax.  Round l >= 1: the fp32 dot v . x, then in float64
//   c = dot / (norm[col] norm[idx]);  c <- (1 - |c|) norm ('pca'), ((1 - c) / 2) norm ('aa'), 1 - |c| ('nmf');
//   iterval *= c;  argmax.  A zero-norm column gives NaN and never wins (the reference's np.argmax would pick it).
#pragma once
#include "pmf_sivm.h"

enum { PMF_GMAP_PCA = 0, PMF_GMAP_AA = 1, PMF_GMAP_NMF = 2 };
enum { PMF_COLSEL_DOT = 3, PMF_COLSEL_SQ = 4, PMF_COLSEL_SQSUM = 5 };   // what colsel_sums accumulates, behind PMF_SIVM_L2 / L1 / COSINE

struct ColselArgs {
  const float* V;          // [mp][np]
  double* st0;             // [np] LAESA: dmin; GMAP: norm
  double* st1;             // [np] GMAP: iterval
  const double* pscore_in; // partials of the previous launch ...
  const int* pidx_in;
  double* pscore_out;      // ... and of this one, [wgs]
  int* pidx_out;
  int* select;             // [k]
  double* scal;            // LAESA: [0] maxd, [1] log(maxd), as SIVM stores them
  int64_t np;
  int m, n;
  int npanels, panels_per_wg;
  int nprev;               // partials of the previous launch to reduce in the prologue (0: none)
  int use_fixed;           // idx = fixed_idx instead of the prologue's argmax
  int fixed_idx;
  int sel_pos;             // >= 0: workgroup 0 writes select[sel_pos] = idx
  int take_maxd;           // LAESA: the best score of the previous (plain) launch is maxd, workgroup 0 stores it
  int plain;               // LAESA: score = dist, state untouched
  int first;               // LAESA: the first recurrence round (dmin = d); GMAP: round 0 (no x)
};

// the fp32 sums of one lane's 4 columns down the m rows, four independent partial sums each:
//   L2 s = sum (v - x)^2;  L1 s = sum |v - x|;  COSINE s = v . x, nn = |v|^2, xx = |x|^2;  DOT s = v . x;
//   SQ nn = |v|^2;  SQSUM nn = |v|^2, s = sum v  (SQ, SQSUM: xs is not read)
template <int MODE>
__device__ __forceinline__ void colsel_sums(const float* vp, int64_t np, int m, const float* xs, f32x4& st, f32x4& nt, float& xt) {
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
  f32x4 n0 = s0, n1 = s0, n2 = s0, n3 = s0;
  float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
  constexpr bool kNeedsX = MODE != PMF_COLSEL_SQ && MODE != PMF_COLSEL_SQSUM;
  auto step = [&](const f32x4 v, const int r, f32x4& s, f32x4& nn, float& xx) {
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
      xx = fmaf(x, x, xx);
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
    step(v0, r + 0, s0, n0, x0);
    step(v1, r + 1, s1, n1, x1);
    step(v2, r + 2, s2, n2, x2);
    step(v3, r + 3, s3, n3, x3);
  }
  if (r < m) step(*reinterpret_cast<const f32x4*>(vp + (int64_t)r * np), r, s0, n0, x0);
  if (r + 1 < m) step(*reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 1) * np), r + 1, s1, n1, x1);
  if (r + 2 < m) step(*reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 2) * np), r + 2, s2, n2, x2);
  st = (s0 + s1) + (s2 + s3);
  nt = (n0 + n1) + (n2 + n3);
  xt = (x0 + x1) + (x2 + x3);
}

// x = V[:, idx] into LDS (idx < 0: the origin)
__device__ __forceinline__ void colsel_stage_x(const float* V, int64_t np, int m, int idx, float* xs) {
  const float* xcol = V + (idx >= 0 ? idx : 0);
  for (int r = threadIdx.x; r < m; r += 256) xs[r] = idx >= 0 ? xcol[(int64_t)r * np] : 0.f;
  __syncthreads();
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_laesa_pass(const ColselArgs a) {
  extern __shared__ float xs[];                 // [m]
  __shared__ double sb[4];
  __shared__ int ib[4];
  const int tid = threadIdx.x;

  // ---- prologue: which column this pass measures against (as k_sivm_pass) -------------------------------------------
  int idx = a.fixed_idx;
  if (a.nprev > 0) {
    double best;
    int bi;
    sivm_reduce_partials(a.pscore_in, a.pidx_in, a.nprev, a.n, sb, ib, &best, &bi);
    if (!a.use_fixed) idx = bi;
    if (a.take_maxd && blockIdx.x == 0 && tid == 0) { a.scal[0] = best; a.scal[1] = log(best); }
  }
  if (blockIdx.x == 0 && tid == 0 && a.sel_pos >= 0) a.select[a.sel_pos] = idx;

  const int c_begin = blockIdx.x * a.panels_per_wg * 64;
  const int c_end = min((blockIdx.x + 1) * a.panels_per_wg, a.npanels) * 64;
  const int nquads = (c_end - c_begin) / 4;
  colsel_stage_x(a.V, a.np, a.m, idx, xs);

  double bs = -INFINITY;
  int bidx = 0x7fffffff;
  for (int q = tid; q < nquads; q += 256) {
    const int c = c_begin + 4 * q;
    f32x4 st, nt;
    float xx;
    colsel_sums<METRIC>(a.V + c, a.np, a.m, xs, st, nt, xx);
    f32x4 dist;
    if (METRIC == PMF_SIVM_L2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) dist[e] = sqrtf(st[e]);
    } else if (METRIC == PMF_SIVM_L1) {
      dist = st;
    } else {
      const float xn = sqrtf(xx);
#pragma unroll
      for (int e = 0; e < 4; ++e) dist[e] = 1.f - st[e] / (sqrtf(nt[e]) * xn + 1e-9f);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c + e >= a.n) continue;
      double d = (double)dist[e];
      if (!a.plain) {
        if (!a.first) {
          const double old = a.st0[c + e];
          d = d < old ? d : old;                // (a NaN d keeps the old minimum)
        }
        a.st0[c + e] = d;
      }
      sivm_better(bs, bidx, d, c + e);
    }
  }
  sivm_wg_best(bs, bidx, sb, ib);
  if (tid == 0) { a.pscore_out[blockIdx.x] = bs; a.pidx_out[blockIdx.x] = bidx; }
}

template <int METHOD>
__global__ __launch_bounds__(256) void k_gmap_pass(const ColselArgs a) {
  extern __shared__ float xs[];                 // [m] (round 0: none)
  __shared__ double sb[4];
  __shared__ int ib[4];
  const int tid = threadIdx.x;

  int idx = 0;
  double norm_x = 1.0;
  if (!a.first) {                               // the column the previous round chose
    double best;
    sivm_reduce_partials(a.pscore_in, a.pidx_in, a.nprev, a.n, sb, ib, &best, &idx);
    if (blockIdx.x == 0 && tid == 0 && a.sel_pos >= 0) a.select[a.sel_pos] = idx;
    norm_x = a.st0[idx];
  }

  const int c_begin = blockIdx.x * a.panels_per_wg * 64;
  const int c_end = min((blockIdx.x + 1) * a.panels_per_wg, a.npanels) * 64;
  const int nquads = (c_end - c_begin) / 4;
  if (!a.first) colsel_stage_x(a.V, a.np, a.m, idx, xs);

  double bs = -INFINITY;
  int bidx = 0x7fffffff;
  if (a.first) {
    const double sqrt_m = sqrt((double)a.m);
    for (int q = tid; q < nquads; q += 256) {
      const int c = c_begin + 4 * q;
      f32x4 st, nt;
      float xx;
      colsel_sums<(METHOD == PMF_GMAP_NMF ? PMF_COLSEL_SQSUM : PMF_COLSEL_SQ)>(a.V + c, a.np, a.m, xs, st, nt, xx);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c + e >= a.n) continue;
        const double nrm = sqrt((double)nt[e]);
        const double it = METHOD == PMF_GMAP_NMF ? 1.0 - (double)st[e] / (sqrt_m * nrm) : nrm;
        a.st0[c + e] = nrm;
        a.st1[c + e] = it;
        sivm_better(bs, bidx, it, c + e);
      }
    }
  } else {
    for (int q = tid; q < nquads; q += 256) {
      const int c = c_begin + 4 * q;
      f32x4 st, nt;
      float xx;
      colsel_sums<PMF_COLSEL_DOT>(a.V + c, a.np, a.m, xs, st, nt, xx);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c + e >= a.n) continue;
        const double nrm = a.st0[c + e];
        double cc = (double)st[e] / (nrm * norm_x);
        if (METHOD == PMF_GMAP_PCA) cc = (1.0 - fabs(cc)) * nrm;
        else if (METHOD == PMF_GMAP_AA) cc = ((cc * -1.0 + 1.0) / 2.0) * nrm;
        else cc = 1.0 - fabs(cc);
        const double it = cc * a.st1[c + e];
        a.st1[c + e] = it;
        sivm_better(bs, bidx, it, c + e);
      }
    }
  }
  sivm_wg_best(bs, bidx, sb, ib);
  if (tid == 0) { a.pscore_out[blockIdx.x] = bs; a.pidx_out[blockIdx.x] = bidx; }
}
