// pmf_chnmf.h -- CHNMF (pymf/chnmf.py:152-191): the random projections proj = R V in float64 and, for every pair (i, j) of its rows,
// the vertices of the 2-D convex hull of the points (proj[i][c], proj[j][c]).  Runs on an AA context with resident dense data.
//
// Projection (k_chnmf_proj): R [16][mp] float64 (rows >= base_sel and columns >= m zero), V read once in float32 and widened,
// products and sums on the float64 MFMA; proj [16][np] float64 stays on the device.
//
// Hull of one pair, two stages, all of it float64:
//   stage 1, the filter.  k_hull_extremes: one sweep over the points in the column-panel decomposition of pmf_colsweep.h (a
//     workgroup owns a contiguous range of 64-column panels) finds the extreme point in D fixed directions (kHullDirs: angles
//     2 pi t / 128, D = 32 takes every fourth; +-x and +-y are among them, exactly) and the largest coordinate magnitude
//     `scale`; argmax as everywhere (sivm_better: lowest index wins, no float atomics, a NaN never wins), partials per
//     workgroup.  k_hull_polygon (one workgroup) reduces the partials to the polygon of the extremes -- convex, counter-clockwise
//     -- and its edges.  k_hull_filter: a second sweep discards every point that lies inside EVERY edge by more than
//     64 2^-53 scale (|ex| + |ey|) in the cross product, i.e. by more than 64 2^-53 scale in distance: the cross product of
//     coordinates <= scale carries an error below 8 2^-53 scale (|ex| + |ey|), and a hull vertex is never strictly inside a
//     polygon of data points, so no hull vertex is discarded.  Survivors are counted per workgroup; k_hull_compact writes them
//     in ascending index order from the prefix sums of the counts (no atomics).
//   stage 2, the exact hull of the survivors.  k_hull_chain (one workgroup): bitonic sort by (x, y, index) in LDS, then the
//     monotone chain with a STRICT turn test (collinear points on an edge are not vertices: the reference's `dists > 0`,
//     chnmf.py:44-45); of bit-identical points only the first of the sorted run -- the lowest index -- is offered, which is the
//     reference's vq (chnmf.py:167: first index among duplicates; every duplicate of a vertex survives the filter with it).
//     The vertices are marked in an n-sized byte mask shared by all pairs.
// Union: k_hull_count + k_hull_compact over the mask give _hull_idx, ascending.
#pragma once
#include "pmf_dev.h"
#include "pmf_colsweep.h"

constexpr int PMF_CH_MAX_SEL = 16;          // base_sel: one tile row of the float64 MFMA
constexpr int PMF_CH_CAP = 4096;            // survivors k_hull_chain takes
constexpr int PMF_CH_D0 = 32;               // directions of the filter; the rerun takes PMF_CH_D1
constexpr int PMF_CH_D1 = 128;
constexpr int PMF_CH_DCHUNK = 32;           // directions a workgroup of k_hull_extremes follows (gridDim.y chunks)
constexpr int PMF_CH_EDGE = 5;              // doubles per edge: px, py, ex, ey, margin

// ---- the D1 directions, compile-time constants: angle 2 pi t / D1, reduced to an octant (Taylor series there), the quadrants by
// exact symmetry so that t = 0, D1 / 4, D1 / 2, 3 D1 / 4 are (1, 0), (0, 1), (-1, 0), (0, -1)
struct HullDirs { double x[PMF_CH_D1], y[PMF_CH_D1]; };
constexpr double hull_sin_small(double a) {
  double term = a, s = a;
  for (int k = 1; k < 12; ++k) { term *= -a * a / ((2.0 * k) * (2.0 * k + 1.0)); s += term; }
  return s;
}
constexpr double hull_cos_small(double a) {
  double term = 1.0, s = 1.0;
  for (int k = 1; k < 12; ++k) { term *= -a * a / ((2.0 * k - 1.0) * (2.0 * k)); s += term; }
  return s;
}
constexpr HullDirs hull_make_dirs() {
  HullDirs d{};
  constexpr double kPi = 3.14159265358979323846;
  constexpr int Q = PMF_CH_D1 / 4;
  for (int t = 0; t < PMF_CH_D1; ++t) {
    const int q = t / Q, r = t % Q;
    double cs = 1.0, sn = 0.0;
    if (r != 0) {
      const double a = 2.0 * kPi * r / PMF_CH_D1;
      if (2 * r <= Q) { cs = hull_cos_small(a); sn = hull_sin_small(a); }
      else { cs = hull_sin_small(kPi / 2 - a); sn = hull_cos_small(kPi / 2 - a); }
    }
    d.x[t] = q == 0 ? cs : q == 1 ? -sn : q == 2 ? -cs : sn;
    d.y[t] = q == 0 ? sn : q == 1 ? cs : q == 2 ? -sn : -cs;
  }
  return d;
}
static __constant__ HullDirs kHullDirs = hull_make_dirs();

// what the sweeps of one pair take
struct HullArgs {
  const double* px;        // the pair's two rows of proj, [np] each
  const double* py;
  int n, npanels, panels_per_wg, wgs;
  int D;                   // directions: PMF_CH_D0 or PMF_CH_D1
  double* pscore;          // [wgs][D] partials of k_hull_extremes ...
  int* pidx;
  double* pmax;            // ... [wgs] largest |coordinate|
  double* edges;           // [D][PMF_CH_EDGE] (k_hull_polygon)
  unsigned char* keep;     // [np] 1: survives the filter
  int* counts;             // [wgs] survivors per workgroup
};

// proj [16][np] = Rp [16][mp] V [mp][np]: wave w of a workgroup owns columns 256 b + 64 w .. + 63, four 16 x 16 accumulators.
// Operand order of v_mfma_f64_16x16x4_f64 (pmf_svd.h): lane l supplies row / column l & 15 at k = l >> 4; C / D: lane l, register r
// <-> row (l >> 4) + 4 r, column l & 15.  m4 = m rounded up to 4 (<= mp: the rows beyond m are zero in both operands).
__global__ __launch_bounds__(256) void k_chnmf_proj(const double* __restrict__ Rp, const float* __restrict__ V, int64_t mp, int np, int m4,
                                                    double* __restrict__ proj) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int c0 = ((int)blockIdx.x * 4 + wv) * 64;
  if (c0 >= np) return;
  f64x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const double* rp = Rp + (int64_t)i * mp + g;
  const float* vp = V + (int64_t)g * np + c0 + i;
  for (int k = 0; k < m4; k += 4) {
    const double a = rp[k];
    float b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = vp[(int64_t)k * np + 16 * j];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mfma_f64(a, (double)b[j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) proj[(int64_t)(g + 4 * r) * np + c0 + 16 * j + i] = acc[j][r];
}

// the workgroup's columns: [c_begin, c_end), pad columns (>= n) cut off
__device__ __forceinline__ void hull_range(const HullArgs& a, int* c_begin, int* c_end) {
  *c_begin = (int)blockIdx.x * a.panels_per_wg * 64;
  *c_end = min(min(((int)blockIdx.x + 1) * a.panels_per_wg, a.npanels) * 64, a.n);
}

// stage 1, first sweep.  grid = (wgs, D / PMF_CH_DCHUNK), 256 threads
__global__ __launch_bounds__(256) void k_hull_extremes(const HullArgs a) {
  __shared__ double sb[4];
  __shared__ int ib[4];
  int c_begin, c_end;
  hull_range(a, &c_begin, &c_end);
  const int stride = PMF_CH_D1 / a.D;                       // D0 takes every fourth direction
  const int t0 = (int)blockIdx.y * PMF_CH_DCHUNK;
  double bs[PMF_CH_DCHUNK];
  int bi[PMF_CH_DCHUNK];
#pragma unroll
  for (int u = 0; u < PMF_CH_DCHUNK; ++u) { bs[u] = -INFINITY; bi[u] = 0x7fffffff; }
  double mx = 0.0;
  for (int c = c_begin + (int)threadIdx.x; c < c_end; c += 256) {
    const double x = a.px[c], y = a.py[c];
    mx = fmax(mx, fmax(fabs(x), fabs(y)));
#pragma unroll
    for (int u = 0; u < PMF_CH_DCHUNK; ++u) {
      const int t = (t0 + u) * stride;
      const double s = kHullDirs.x[t] * x + kHullDirs.y[t] * y;
      if (s > bs[u]) { bs[u] = s; bi[u] = c; }              // (c ascends: the first -- lowest -- column attaining the score stays)
    }
  }
#pragma unroll
  for (int u = 0; u < PMF_CH_DCHUNK; ++u) {
    double s = bs[u];
    int i = bi[u];
    sivm_wg_best(s, i, sb, ib);
    if (threadIdx.x == 0) {
      a.pscore[(int64_t)blockIdx.x * a.D + t0 + u] = s;
      a.pidx[(int64_t)blockIdx.x * a.D + t0 + u] = i;
    }
  }
  if (blockIdx.y == 0) {
    int none = 0;
    sivm_wg_best(mx, none, sb, ib);
    if (threadIdx.x == 0) a.pmax[blockIdx.x] = mx;
  }
}

// the polygon of the extremes and its edges.  One workgroup of 256 threads; D divides 256.
__global__ __launch_bounds__(256) void k_hull_polygon(const HullArgs a) {
  __shared__ double ss[256];
  __shared__ int si[256];
  __shared__ double vx[PMF_CH_D1], vy[PMF_CH_D1];
  __shared__ double sb[4];
  __shared__ int ib[4];
  __shared__ int nedges;
  const int D = a.D, t = (int)threadIdx.x % D, grp = (int)threadIdx.x / D, ngrp = 256 / D;
  if (threadIdx.x == 0) nedges = 0;
  double s = -INFINITY;
  int i = 0x7fffffff;
  for (int w = grp; w < a.wgs; w += ngrp) sivm_better(s, i, a.pscore[(int64_t)w * D + t], a.pidx[(int64_t)w * D + t]);
  ss[threadIdx.x] = s; si[threadIdx.x] = i;
  double mx = 0.0;
  for (int w = (int)threadIdx.x; w < a.wgs; w += 256) mx = fmax(mx, a.pmax[w]);
  int none = 0;
  sivm_wg_best(mx, none, sb, ib);                           // (its barriers also publish ss / si)
  const double scale = sb[0];
  if ((int)threadIdx.x < D) {
    for (int q = 1; q < ngrp; ++q) sivm_better(s, i, ss[q * D + t], si[q * D + t]);
    const int idx = ((unsigned)i < (unsigned)a.n) ? i : 0;  // no finite score at all: column 0, nothing is read from outside proj
    vx[t] = a.px[idx]; vy[t] = a.py[idx];
  }
  __syncthreads();
  if ((int)threadIdx.x < D) {
    const int t1 = t + 1 < D ? t + 1 : 0;
    const double ex = vx[t1] - vx[t], ey = vy[t1] - vy[t];
    const bool degenerate = ex == 0.0 && ey == 0.0;         // both directions found the same point: no edge, every point passes
    double* e = a.edges + t * PMF_CH_EDGE;
    e[0] = vx[t]; e[1] = vy[t]; e[2] = ex; e[3] = ey;
    e[4] = degenerate ? -INFINITY : 64.0 * 0x1p-53 * scale * (fabs(ex) + fabs(ey));
    if (!degenerate) nedges = 1;                            // (every writer stores the same value)
  }
  __syncthreads();
  if (threadIdx.x == 0 && nedges == 0) a.edges[4] = INFINITY;   // one distinct point: no polygon, nothing is discarded
}

// the number of set flags among the workgroup's 256 threads in every thread; *before: among the threads below this one
__device__ __forceinline__ int hull_wg_count(bool flag, int* wsum, int* before) {
  const unsigned long long b = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  int pre = __popcll(b & ((1ull << lane) - 1ull)), tot = 0;
  for (int w = 0; w < 4; ++w) { if (w < wave) pre += wsum[w]; tot += wsum[w]; }
  *before = pre;
  return tot;
}

// stage 1, second sweep: keep[c] for the workgroup's columns (pad columns: 0), counts[wg]
__global__ __launch_bounds__(256) void k_hull_filter(const HullArgs a) {
  __shared__ double ed[PMF_CH_D1 * PMF_CH_EDGE];
  __shared__ int wsum[4];
  for (int q = threadIdx.x; q < a.D * PMF_CH_EDGE; q += 256) ed[q] = a.edges[q];
  __syncthreads();
  const int c_begin = (int)blockIdx.x * a.panels_per_wg * 64;
  const int c_pad = min(((int)blockIdx.x + 1) * a.panels_per_wg, a.npanels) * 64;
  int total = 0;
  for (int c0 = c_begin; c0 < c_pad; c0 += 256) {           // (uniform trip count: barriers inside)
    const int c = c0 + (int)threadIdx.x;
    bool kept = false;
    if (c < c_pad) {
      if (c < a.n) {
        const double x = a.px[c], y = a.py[c];
        bool inside = true;
        for (int t = 0; t < a.D; ++t) {
          const double* e = ed + t * PMF_CH_EDGE;
          const double cr = e[2] * (y - e[1]) - e[3] * (x - e[0]);
          inside = inside && (cr > e[4]);                   // (a NaN coordinate is never inside)
        }
        kept = !inside;
      }
      a.keep[c] = kept ? 1 : 0;
    }
    int before;
    total += hull_wg_count(kept, wsum, &before);
  }
  if (threadIdx.x == 0) a.counts[blockIdx.x] = total;
}

// counts[wg] of a byte array (the union mask), same partition
__global__ __launch_bounds__(256) void k_hull_count(const unsigned char* __restrict__ flags, int npanels, int panels_per_wg, int* __restrict__ counts) {
  __shared__ int wsum[4];
  const int c_begin = (int)blockIdx.x * panels_per_wg * 64;
  const int c_pad = min(((int)blockIdx.x + 1) * panels_per_wg, npanels) * 64;
  int total = 0;
  for (int c0 = c_begin; c0 < c_pad; c0 += 256) {
    const int c = c0 + (int)threadIdx.x;
    int before;
    total += hull_wg_count(c < c_pad && flags[c] != 0, wsum, &before);
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// out[0 .. min(total, cap)) = the columns with a set flag, ascending: the workgroup's first position is the sum of the counts of
// the workgroups before it; *total_out = the number of set flags (may exceed cap: nothing is written beyond it)
__global__ __launch_bounds__(256) void k_hull_compact(const unsigned char* __restrict__ flags, const int* __restrict__ counts, int wgs, int npanels,
                                                      int panels_per_wg, int cap, int* __restrict__ out, int* __restrict__ total_out) {
  __shared__ int wsum[4];
  __shared__ int red[2][4];
  int below = 0, all = 0;
  for (int w = threadIdx.x; w < wgs; w += 256) {
    const int v = counts[w];
    all += v;
    if (w < (int)blockIdx.x) below += v;
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { below += __shfl_xor(below, x); all += __shfl_xor(all, x); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = below; red[1][threadIdx.x >> 6] = all; }
  __syncthreads();
  int pos = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  if (blockIdx.x == 0 && threadIdx.x == 0) *total_out = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  const int c_begin = (int)blockIdx.x * panels_per_wg * 64;
  const int c_pad = min(((int)blockIdx.x + 1) * panels_per_wg, npanels) * 64;
  for (int c0 = c_begin; c0 < c_pad; c0 += 256) {
    const int c = c0 + (int)threadIdx.x;
    const bool f = c < c_pad && flags[c] != 0;
    int before;
    const int tot = hull_wg_count(f, wsum, &before);
    if (f && pos + before < cap) out[pos + before] = c;
    pos += tot;
  }
}

// mask[idx[q]] = 1, q < cnt (the vertices a pair's hull was given on the host); indices outside [0, n) are skipped
__global__ __launch_bounds__(256) void k_hull_scatter(const int* __restrict__ idx, int cnt, int n, unsigned char* __restrict__ mask) {
  const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (q < cnt && (unsigned)idx[q] < (unsigned)n) mask[idx[q]] = 1;
}

// (x, y, index) ascending
__device__ __forceinline__ bool hull_less(double xa, double ya, int ia, double xb, double yb, int ib) {
  return xa < xb || (xa == xb && (ya < yb || (ya == yb && ia < ib)));
}

constexpr size_t hull_chain_smem(int P) { return (size_t)P * (2 * sizeof(double) + 3 * sizeof(int)); }

// stage 2.  One workgroup of 1024 threads; dynamic LDS hull_chain_smem(P), P = the power of two >= cap (cap <= PMF_CH_CAP).
// More than cap survivors: nothing is done (the host reads *nsurv and takes another route).
__global__ __launch_bounds__(1024) void k_hull_chain(const double* __restrict__ px, const double* __restrict__ py, const int* __restrict__ surv,
                                                     const int* __restrict__ nsurv, int cap, int P, int n, unsigned char* __restrict__ mask) {
  extern __shared__ double chain_smem[];
  double* xs = chain_smem;
  double* ys = xs + P;
  int* id = reinterpret_cast<int*>(ys + P);
  int* lo = id + P;                                         // the two chains' stacks (positions of the sorted order)
  int* up = lo + P;
  __shared__ int nlo, nup;
  const int cnt = *nsurv;
  if (cnt > cap || cnt > P || cnt < 1) return;              // (uniform)
  int S = 1;
  while (S < cnt) S <<= 1;                                  // S <= P
  for (int q = threadIdx.x; q < S; q += 1024) {
    int c = q < cnt ? surv[q] : 0x7fffffff;
    if (q < cnt && (unsigned)c >= (unsigned)n) c = 0;       // (cannot happen: k_hull_compact writes columns < n)
    xs[q] = q < cnt ? px[c] : INFINITY;
    ys[q] = q < cnt ? py[c] : INFINITY;
    id[q] = c;
  }
  __syncthreads();
  for (int k = 2; k <= S; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < S / 2; t += 1024) {
        const int i0 = ((t & ~(j - 1)) << 1) | (t & (j - 1)), i1 = i0 | j;
        const bool asc = (i0 & k) == 0;
        const double x0 = xs[i0], y0 = ys[i0], x1 = xs[i1], y1 = ys[i1];
        const int d0 = id[i0], d1 = id[i1];
        if (hull_less(x1, y1, d1, x0, y0, d0) == asc) {
          xs[i0] = x1; ys[i0] = y1; id[i0] = d1;
          xs[i1] = x0; ys[i1] = y0; id[i1] = d0;
        }
      }
      __syncthreads();
    }
  // the monotone chain, strict turns; wave 0 builds the lower chain left to right, wave 1 the upper one right to left.  Of a run
  // of equal points only its first position is offered.
  if (threadIdx.x == 0 || threadIdx.x == 64) {
    const bool lower = threadIdx.x == 0;
    int* st = lower ? lo : up;
    int sz = 0;
    for (int q = 0; q < cnt; ++q) {
      const int p = lower ? q : cnt - 1 - q;
      if (p > 0 && xs[p] == xs[p - 1] && ys[p] == ys[p - 1]) continue;
      const double x = xs[p], y = ys[p];
      while (sz >= 2) {
        const int b = st[sz - 1], o = st[sz - 2];
        const double cr = (xs[b] - xs[o]) * (y - ys[o]) - (ys[b] - ys[o]) * (x - xs[o]);
        if (cr <= 0.0) --sz; else break;
      }
      st[sz++] = p;                                         // sz <= cnt <= P
    }
    if (lower) nlo = sz; else nup = sz;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < nlo; q += 1024) mask[id[lo[q]]] = 1;
  for (int q = threadIdx.x; q < nup; q += 1024) mask[id[up[q]]] = 1;
}
