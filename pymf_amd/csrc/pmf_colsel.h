// pmf_colsel.h -- LAESA (pymf/laesa.py) and GMAP (pymf/gmap.py, robust_map = False): the two column selections that sweep the
// data like SIVM's update_w but carry a lighter recurrence.  They run on a SIVM context (pmf_set_option "sivm_rule"), on the
// sweep of pmf_colsweep.h (work decomposition, fp32 sums, argmax chain) and SIVM's buffers; k_sivm_close does the last reduce,
// k_sivm_gather writes W.
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

struct ColselArgs : ColsweepPickArgs {   // (GMAP: of the prologue's fields select and sel_pos only)
  double* st0;             // [np] LAESA: dmin; GMAP: norm
  double* st1;             // [np] GMAP: iterval
  int plain;               // LAESA: score = dist, state untouched
  int first;               // LAESA: the first recurrence round (dmin = d); GMAP: round 0 (no x, no previous launch)
};

template <int METRIC>
__global__ __launch_bounds__(256) void k_laesa_pass(const ColselArgs a) {
  extern __shared__ float xs[];                 // [m]
  __shared__ double sb[4];
  __shared__ int ib[4];
  double log_maxd;
  colsweep_stage_x(a, colsweep_pick(a, sb, ib, &log_maxd), xs);

  double bs = -INFINITY;
  int bidx = 0x7fffffff;
  colsweep_quads(a, [&](const int c) __attribute__((always_inline)) {
    f32x4 st, nt;
    float xx;
    colsweep_sums<METRIC>(a, c, xs, st, nt, xx);
    const f32x4 dist = colsweep_dist<METRIC>(st, nt, xx);
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
  });
  colsweep_finish(a, bs, bidx, sb, ib);
}

template <int METHOD>
__global__ __launch_bounds__(256) void k_gmap_pass(const ColselArgs a) {
  extern __shared__ float xs[];                 // [m] (round 0: none)
  __shared__ double sb[4];
  __shared__ int ib[4];
  int idx = 0;
  if (!a.first) {                               // the column the previous round chose
    double best;
    sivm_reduce_partials(a.pscore_in, a.pidx_in, a.nprev, a.n, sb, ib, &best, &idx);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.sel_pos >= 0) a.select[a.sel_pos] = idx;
  }

  double bs = -INFINITY;
  int bidx = 0x7fffffff;
  if (a.first) {
    const double sqrt_m = sqrt((double)a.m);
    colsweep_quads(a, [&](const int c) __attribute__((always_inline)) {
      f32x4 st, nt;
      float xx;
      colsweep_sums<(METHOD == PMF_GMAP_NMF ? PMF_COLSEL_SQSUM : PMF_COLSEL_SQ)>(a, c, xs, st, nt, xx);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c + e >= a.n) continue;
        const double nrm = sqrt((double)nt[e]);
        const double it = METHOD == PMF_GMAP_NMF ? 1.0 - (double)st[e] / (sqrt_m * nrm) : nrm;
        a.st0[c + e] = nrm;
        a.st1[c + e] = it;
        sivm_better(bs, bidx, it, c + e);
      }
    });
  } else {
    const double norm_x = a.st0[idx];
    colsweep_stage_x(a, idx, xs);
    colsweep_quads(a, [&](const int c) __attribute__((always_inline)) {
      f32x4 st, nt;
      float xx;
      colsweep_sums<PMF_COLSEL_DOT>(a, c, xs, st, nt, xx);
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
    });
  }
  colsweep_finish(a, bs, bidx, sb, ib);
}
