// pmf_sivm.h -- SIVM (pymf/sivm.py): simplex volume maximisation, the column selection of update_w and the multiplier search
// of the simplex-constrained H step.
//
// update_w (sivm.py:145-201) is num_bases + 2 ('fastmap') or num_bases ('origin') dependent passes over V [mp][np]: the
// distance of every column to ONE selected column x = V[:, idx], a pointwise recurrence on three float64 arrays, an argmax.
// k_sivm_pass<METRIC> is one such pass on the sweep of pmf_colsweep.h (work decomposition, fp32 sums, argmax chain).  The
// distance is formed from the difference, as dist.py:57-63 does:  l2 sqrt(sum (v - x)^2),  l1 sum |v - x|,
// cosine 1 - v.x / (|v| |x| + 1e-9).  Recurrence (sivm.py:181-190, float64; sivm_recur), d = log(dist + 1e-8):
//   d_i_times_d_j += d d_sum;  d_sum += d;  d_square += d^2;  score = d_i_times_d_j + a d_sum - (l / 2) d_square
// with a = log(maxd).  The three fastmap passes (sivm.py:153-155) run the same kernel "plain": score = dist, state untouched;
// behind the last of them workgroup 0 writes maxd and a.  k_sivm_close does the last reduce, k_sivm_gather writes
// W = V[:, select] (a -1 entry is a Python index there: the LAST data column).
// The same selection among the ROWS of a row-major matrix, whose samples are too long for LDS, is the long-sample pass
// further down (k_sivm_rowdist, k_sivm_rowstep): SIVM_CUR's row selection.
#pragma once
#include "pmf_colsweep.h"

constexpr int PMF_SIVM_MAX_M = 16384;   // x is staged whole in LDS (m floats of dynamic shared memory: 64 KiB at the limit)

struct SivmArgs : ColsweepPickArgs {
  double* dij;             // [np] d_i_times_d_j
  double* dsum;            // [np] d_sum
  double* dsq;             // [np] d_square
  int plain;               // score = dist, state untouched
  int l;                   // step of the recurrence (sivm.py:181)
};

// candidate i's step of the recurrence: its three states updated, its score returned
__device__ __forceinline__ double sivm_recur(double dist, double a_log, double hl, double* dij, double* dsum, double* dsq, int i) {
  const double d = log(dist + 1e-8);
  const double ds_old = dsum[i];
  const double ij = dij[i] + d * ds_old;
  const double ds = ds_old + d;
  const double dq = dsq[i] + d * d;
  dij[i] = ij;
  dsum[i] = ds;
  dsq[i] = dq;
  return ij + a_log * ds - hl * dq;
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_sivm_pass(const SivmArgs a) {
  extern __shared__ float xs[];                 // [m]
  __shared__ double sb[4];
  __shared__ int ib[4];
  double a_log;
  const int idx = colsweep_pick(a, sb, ib, &a_log);
  if (!a.take_maxd && !a.plain) a_log = a.scal[1];
  const double hl = 0.5 * (double)a.l;
  colsweep_stage_x(a, idx, xs);

  double bs = -INFINITY;
  int bidx = 0x7fffffff;
  colsweep_quads(a, [&](const int c) __attribute__((always_inline)) {
    f32x4 st, nt;
    float xx;
    colsweep_sums<METRIC>(a, c, xs, st, nt, xx);
    const f32x4 dist = colsweep_dist<METRIC>(st, nt, xx);
    if (a.plain) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < a.n) sivm_better(bs, bidx, (double)dist[e], c + e);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < a.n) sivm_better(bs, bidx, sivm_recur((double)dist[e], a_log, hl, a.dij, a.dsum, a.dsq, c + e), c + e);
    }
  });
  colsweep_finish(a, bs, bidx, sb, ib);
}

// the reduce behind the last pass: select[sel_pos] (and maxd, a when no recurrence pass followed the plain ones: num_bases = 1)
__global__ __launch_bounds__(256) void k_sivm_close(const double* __restrict__ ps, const int* __restrict__ pi, int count, int n, int sel_pos,
                                                    int take_maxd, int origin_first, int* __restrict__ select, double* __restrict__ scal) {
  __shared__ double sb[4];
  __shared__ int ib[4];
  double best;
  int idx;
  sivm_reduce_partials(ps, pi, count, n, sb, ib, &best, &idx);
  if (threadIdx.x == 0) {
    select[sel_pos] = origin_first ? -1 : idx;
    if (take_maxd) { scal[0] = best; scal[1] = log(best); }
  }
}

// W [mp][KP] = V[:, select] in selection order; -1 is the last data column (a Python index, sivm.py:198); padding zero
__global__ __launch_bounds__(256) void k_sivm_gather(const float* __restrict__ V, int64_t np, int m, int n, int k, int KP, int64_t elems,
                                                     const int* __restrict__ select, float* __restrict__ W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= elems) return;
  const int64_t r = i / KP;
  const int j = (int)(i % KP);
  float w = 0.f;
  if (r < m && j < k) {
    int s = select[j];
    if (s < 0) s += n;
    s = min(max(s, 0), n - 1);
    w = V[r * np + s];
  }
  W[i] = w;
}

// ---- the long-sample pass: SIVM among the ROWS of a row-major A [C][ld] (SIVM_CUR's row selection) ------------
// The C <= 16 384 rows are the candidates, the R valid columns their dimension (64 x 1 048 576: 64 candidates of dimension one
// million, which k_sivm_pass cannot stage).  One round is two launches:
//   k_sivm_rowdist<METRIC>  grid (column slabs of PMF_SIVM_SLAB) x (blocks of PMF_SIVM_ROWS_WG rows): one read of A.  The slab's
//                           piece of x = A[idx, :] (idx = *cur; -1: the origin, zeros) is staged in LDS once per workgroup; each of
//                           the four waves owns PMF_SIVM_ROWS_WAVE rows and walks the slab 256 columns at a time, 16 bytes per lane,
//                           coalesced along the row, one x read from LDS serving its eight rows.  Products and differences are fp32;
//                           a fp32 running sum covers a lane's share of one slab of one row -- at most 32 terms (8 steps of 4
//                           columns), the longest fp32 sum of this pass.  Everything above is float64 in a fixed order: the 64
//                           lanes (xor butterfly), then the slabs (k_sivm_rowstep).  Partials [slab][row]: the distance sum (l2: of
//                           squares, l1: of moduli; cosine: v.x and, behind it, |v|^2; |x|^2 per slab).  Rows >= C are never
//                           written, columns >= R are masked to zero whatever the padding holds.
//   k_sivm_rowstep          one workgroup: per row the slab partials in float64 (tpr threads of a row take every tpr-th slab in
//                           ascending order, then an xor butterfly), dist (l2 sqrt, cosine 1 - v.x / (|v||x| + 1e-9), in float64),
//                           the recurrence of k_sivm_pass and the argmax (sivm_better, sivm_wg_best); thread 0 leaves idx in *cur
//                           for the next launch, appends to select[] and, behind the last plain pass, stores maxd and a.
// No host read between rounds, no float atomics, two runs give the same bits.
constexpr int PMF_SIVM_ROW_MAX_C = 16384;  // candidates of the long-sample pass (one workgroup does the score step)
constexpr int PMF_SIVM_SLAB = 2048;        // columns per slab: 8 KiB of x in LDS, 8 steps of 256 columns
constexpr int PMF_SIVM_ROWS_WAVE = 8;      // rows a wave carries through its slab
constexpr int PMF_SIVM_ROWS_WG = 4 * PMF_SIVM_ROWS_WAVE;

struct SivmRowArgs {
  const float* A;          // [>= C rows][ld]
  int64_t ld;
  const int* cur;          // [1] the row this round measures against (-1: the origin)
  double* part;            // [slabs][Cs]; cosine: a second block of the same size behind it
  double* xpart;           // [slabs] |x|^2 (cosine)
  int C, R, Cs, slabs;
};

// the sum of s over the 64 lanes in float64, a fixed order, the same bits in every lane
__device__ __forceinline__ double sivm_wave_sum(double s) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) s += __shfl_xor(s, x);
  return s;
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_sivm_rowdist(const SivmRowArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[PMF_SIVM_SLAB];
  __shared__ double xw[4];
  constexpr int NR = PMF_SIVM_ROWS_WAVE;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slab = blockIdx.x;
  const int c0 = slab * PMF_SIVM_SLAB;
  const int R = a.R, C = a.C;
  const int64_t ld = a.ld;
  const int idx = min(*a.cur, C - 1);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // ---- the slab's piece of x into LDS (columns >= R: zero) ----------------------------------------------------------
  {
    const float* xrow = a.A + (int64_t)max(idx, 0) * ld;
    float xx = 0.f;
#pragma unroll
    for (int q = 0; q < PMF_SIVM_SLAB / 1024; ++q) {
      const int o = 4 * (tid + 256 * q), c = c0 + o;
      f32x4 x = zero;
      if (idx >= 0 && c < R) {
        x = *reinterpret_cast<const f32x4*>(xrow + c);
        if (c + 4 > R) {
#pragma unroll
          for (int e = 1; e < 4; ++e)
            if (c + e >= R) x[e] = 0.f;
        }
      }
      *reinterpret_cast<f32x4*>(xs + o) = x;
      if (METRIC == PMF_SIVM_COSINE) xx += (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]);
    }
    if (METRIC == PMF_SIVM_COSINE) {               // |x|^2 of the slab: lanes, then waves, float64
      const double w = sivm_wave_sum((double)xx);
      if (lane == 0) xw[wave] = w;
    }
    __syncthreads();
    if (METRIC == PMF_SIVM_COSINE && blockIdx.y == 0 && tid == 0) a.xpart[slab] = ((xw[0] + xw[1]) + xw[2]) + xw[3];
  }

  // ---- the wave's rows through the slab -------------------------------------------------------------------------------
  const int r0 = blockIdx.y * PMF_SIVM_ROWS_WG + wave * NR;
  const float* rp[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) rp[j] = a.A + (int64_t)min(r0 + j, C - 1) * ld;   // (rows >= C reread the last row; never written)
  f32x4 s[NR], nn[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) { s[j] = zero; nn[j] = zero; }
  for (int st = 0; st < PMF_SIVM_SLAB / 256; ++st) {
    const int cb = c0 + 256 * st;
    if (cb >= R) break;                            // (uniform)
    const int c = cb + 4 * lane;
    const f32x4 x = *reinterpret_cast<const f32x4*>(xs + 256 * st + 4 * lane);
    f32x4 v[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) v[j] = c < R ? *reinterpret_cast<const f32x4*>(rp[j] + c) : zero;
    if (c < R && c + 4 > R) {                      // the ragged last quad: columns >= R do not contribute
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 1; e < 4; ++e)
          if (c + e >= R) v[j][e] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      if (METRIC == PMF_SIVM_L2) {
        const f32x4 d = v[j] - x;
        s[j] += d * d;
      } else if (METRIC == PMF_SIVM_L1) {
        const f32x4 d = v[j] - x;
#pragma unroll
        for (int e = 0; e < 4; ++e) s[j][e] += fabsf(d[e]);
      } else {
        s[j] += v[j] * x;
        nn[j] += v[j] * v[j];
      }
    }
  }

  // ---- lanes in float64; lane j writes row r0 + j ---------------------------------------------------------------------
  double out = 0.0, out2 = 0.0;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const double t = sivm_wave_sum((double)((s[j][0] + s[j][1]) + (s[j][2] + s[j][3])));
    if (lane == j) out = t;
    if (METRIC == PMF_SIVM_COSINE) {
      const double t2 = sivm_wave_sum((double)((nn[j][0] + nn[j][1]) + (nn[j][2] + nn[j][3])));
      if (lane == j) out2 = t2;
    }
  }
  if (lane < NR && r0 + lane < C) {
    const int64_t o = (int64_t)slab * a.Cs + r0 + lane;
    a.part[o] = out;
    if (METRIC == PMF_SIVM_COSINE) a.part[(int64_t)a.slabs * a.Cs + o] = out2;
  }
}

struct SivmRowStepArgs {
  const double* part;      // as SivmRowArgs
  const double* xpart;
  double* dij;             // [C] the recurrence's state
  double* dsum;
  double* dsq;
  int* cur;                // [1] in: the row this round measured against; out: the row of the next round
  int* select;             // [nsel]
  double* scal;            // [0] maxd, [1] a = log(maxd)
  int C, Cs, slabs;
  int metric;
  int tpr;                 // threads per row of the slab sum: a power of two <= 64
  int plain;               // score = dist, state untouched
  int l;                   // step of the recurrence (sivm.py:181)
  int take_maxd;           // this is the last plain pass: its best score is maxd
  int keep_cur;            // the next round measures against the same row ('origin': -1 again)
  int sel_pos;             // >= 0: select[sel_pos] = the row this round measured against
  int last_pos;            // >= 0: select[last_pos] = the row of the next round (the last launch)
};

__global__ __launch_bounds__(256) void k_sivm_rowstep(const SivmRowStepArgs a) {
  __shared__ double sb[4];
  __shared__ int ib[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tpr = a.tpr, ql = tid & (tpr - 1), g = tid / tpr, groups = 256 / tpr;
  const int C = a.C;
  const int cur_in = *a.cur;
  const bool cosine = a.metric == PMF_SIVM_COSINE;
  const int64_t blk = (int64_t)a.slabs * a.Cs;

  double xn = 0.0;                                 // cosine: |x| from the slabs' |x|^2 (threads, lanes, waves: a fixed order)
  if (cosine) {
    double t = 0.0;
    for (int q = tid; q < a.slabs; q += 256) t += a.xpart[q];
    t = sivm_wave_sum(t);
    if (lane == 0) sb[wave] = t;
    __syncthreads();
    xn = sqrt(((sb[0] + sb[1]) + sb[2]) + sb[3]);
    __syncthreads();
  }
  const double a_log = a.plain ? 0.0 : a.scal[1];
  const double hl = 0.5 * (double)a.l;
  double bs = -INFINITY;
  int bi = 0x7fffffff;
  for (int rb = 0; rb < C; rb += groups) {         // (uniform trip count: the shuffles below are executed by every lane)
    const int r = rb + g;
    double s0 = 0.0, s1 = 0.0;
    if (r < C) {
      const double* p = a.part + r;
      for (int q = ql; q < a.slabs; q += tpr) {
        s0 += p[(int64_t)q * a.Cs];
        if (cosine) s1 += p[blk + (int64_t)q * a.Cs];
      }
    }
    for (int x = 1; x < tpr; x <<= 1) {
      s0 += __shfl_xor(s0, x);
      s1 += __shfl_xor(s1, x);
    }
    if (r < C && ql == 0) {
      double dist;
      if (a.metric == PMF_SIVM_L2) dist = sqrt(s0);
      else if (a.metric == PMF_SIVM_L1) dist = s0;
      else dist = 1.0 - s0 / (sqrt(s1) * xn + 1e-9);
      if (a.plain) sivm_better(bs, bi, dist, r);
      else sivm_better(bs, bi, sivm_recur(dist, a_log, hl, a.dij, a.dsum, a.dsq, r), r);
    }
  }
  sivm_wg_best(bs, bi, sb, ib);
  if (tid == 0) {
    const double best = sb[0];
    const int arg = ((unsigned)ib[0] < (unsigned)C) ? ib[0] : 0;   // (no finite score at all: row 0, nothing outside A is read)
    const int next = a.keep_cur ? cur_in : arg;
    if (a.sel_pos >= 0) a.select[a.sel_pos] = cur_in;
    if (a.take_maxd) { a.scal[0] = best; a.scal[1] = log(best); }
    if (a.last_pos >= 0) a.select[a.last_pos] = next;
    *a.cur = next;
  }
}

// ---- the H step (aa.py:93-111): min 1/2 x^T (W^T W) x - (W^T v)^T x, x >= 0, sum x = 1, one problem per column ---------------
// For a fixed multiplier lambda this is the non-negative QP with right-hand side f + lambda 1 (solve_nnqps); sum x(lambda) is
// continuous, non-decreasing and piecewise linear, so a bracketing secant (Illinois) on sum x(lambda) - 1 ends after finitely
// many rounds: lambda = -max_j f_j gives x = 0, the upper end is grown until sum x >= 1.

// S = W^T W in float64 from the float32 W, [KP][KP], the identity on the padding (what the QP kernels expect)
__global__ __launch_bounds__(256) void k_sivm_hessian(const float* __restrict__ W, int m, int k, int KP, double* __restrict__ Gd) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= KP * KP) return;
  const int i = e / KP, j = e % KP;
  double s = 0.0;
  if (i < k && j < k) {
    for (int r = 0; r < m; ++r) s = fma((double)W[(int64_t)r * KP + i], (double)W[(int64_t)r * KP + j], s);
  } else {
    s = i == j ? 1.0 : 0.0;
  }
  Gd[e] = s;
}

struct SivmLamArgs {
  const float* PS;         // [KP][ldp]: row j, column c = (W^T v_c)_j
  int64_t ldp;
  float* F;                // [KP][np]: f + lambda
  const float* X;          // [KP][np]
  const double* Gd;        // [KP][KP] W^T W
  const double* Binv;      // [KP][KP] its inverse
  double* st;              // [6][np]: lam_min, lo, g_lo, hi, g_hi, lam
  int* side;               // [np]: 0 no upper end yet; otherwise -1 / +1 = the end the last round replaced (lower / upper)
  int* unfinished;         // [rounds + 1]
  int64_t np;
  int n, k, KP, round;
  double tol;
};

// round 0: the bracket's lower end and the first multiplier -- the one of the equality-constrained problem without the
// signs, lambda = (1 - 1^T inv(S) f) / (1^T inv(S) 1) (exact for a column inside the simplex); where that is not above the
// lower end, lambda_min + S_jj at j = argmax f (x = e_j: sum x = 1 if no other variable enters)
__global__ __launch_bounds__(256) void k_sivm_lam_init(const SivmLamArgs a) {
  __shared__ double u[64];
  __shared__ double usum;
  if (threadIdx.x < 64) {
    double s = 0.0;
    if ((int)threadIdx.x < a.k)
      for (int j = 0; j < a.k; ++j) s += a.Binv[(int64_t)threadIdx.x * a.KP + j];
    u[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int j = 0; j < a.k; ++j) s += u[j];
    usum = s;
  }
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.np) return;
  if (c >= a.n) {
    for (int j = 0; j < a.KP; ++j) a.F[(int64_t)j * a.np + c] = 0.f;
    return;
  }
  double fmax = -INFINITY, uf = 0.0;
  int jmax = 0;
  for (int j = 0; j < a.k; ++j) {
    const double f = (double)a.PS[(int64_t)j * a.ldp + c];
    if (f > fmax) { fmax = f; jmax = j; }
    uf = fma(u[j], f, uf);
  }
  const double lam_min = -fmax;
  double lam = (1.0 - uf) / usum;
  if (!(usum > 0.0) || !(lam > lam_min)) lam = lam_min + a.Gd[(int64_t)jmax * a.KP + jmax];
  a.st[0 * a.np + c] = lam_min;
  a.st[1 * a.np + c] = lam_min;
  a.st[2 * a.np + c] = -1.0;
  a.st[3 * a.np + c] = lam_min;
  a.st[4 * a.np + c] = 0.0;
  a.st[5 * a.np + c] = lam;
  a.side[c] = 0;
  for (int j = 0; j < a.KP; ++j)
    a.F[(int64_t)j * a.np + c] = j < a.k ? (float)((double)a.PS[(int64_t)j * a.ldp + c] + lam) : 0.f;
}

// behind a round's solve: g = sum x - 1; a column within tol is finished (its multiplier and right-hand side stay); the
// others move their bracket and multiplier, write the new right-hand side and count themselves in unfinished[round]
__global__ __launch_bounds__(256) void k_sivm_lam_update(const SivmLamArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.n) return;
  double s = 0.0;
  for (int j = 0; j < a.k; ++j) s += (double)a.X[(int64_t)j * a.np + c];
  const double g = s - 1.0;
  if (fabs(g) <= a.tol) return;
  atomicAdd(a.unfinished + a.round, 1);
  const double lam_min = a.st[0 * a.np + c];
  double lo = a.st[1 * a.np + c], glo = a.st[2 * a.np + c], hi = a.st[3 * a.np + c], ghi = a.st[4 * a.np + c];
  double lam = a.st[5 * a.np + c];
  int side = a.side[c];
  if (g < 0.0) {
    lo = lam; glo = g;
    if (side < 0) ghi *= 0.5;             // the lower end moved twice running: Illinois halves the other end's value
    if (side != 0) side = -1;
  } else {
    hi = lam; ghi = g;
    if (side > 0) glo *= 0.5;
    side = 1;
  }
  if (side == 0) {
    lam = lam + 2.0 * (lam - lam_min);    // no upper end yet: grow
  } else {
    double nl = (lo * ghi - hi * glo) / (ghi - glo);
    if (!(nl > lo && nl < hi)) nl = 0.5 * (lo + hi);
    lam = nl;
  }
  a.st[1 * a.np + c] = lo; a.st[2 * a.np + c] = glo; a.st[3 * a.np + c] = hi; a.st[4 * a.np + c] = ghi;
  a.st[5 * a.np + c] = lam;
  a.side[c] = side;
  for (int j = 0; j < a.k; ++j) a.F[(int64_t)j * a.np + c] = (float)((double)a.PS[(int64_t)j * a.ldp + c] + lam);
}
