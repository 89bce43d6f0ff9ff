// pmf_vq.h -- vq / pdist (pymf/dist.py:107-130): every column of the resident V [mp][np] against nq <= 128 query vectors in ONE
// sweep, the nearest column per query (pmf_vq_columns) or the whole nq x n distance block and the nearest query per column
// (pmf_vq_assign).
//
// k_vq_pass<METRIC> runs on the sweep of pmf_colsweep.h: a workgroup owns a contiguous range of 64-column panels
// (ColsweepArgs, panel_partition; colsweep_quads_uniform: colsweep_quads with uniform trips, since the body holds barriers), a
// lane 4 adjacent columns with one 16-byte read per row.  The queries sit in LDS as
// [rows][QL] (QP = nq padded to a multiple of 16; pad queries are zero vectors, computed and never read back) and are read as a
// broadcast: every lane of a wave the same 16 bytes, four queries per ds_read_b128, no bank conflict.  A lane carries the
// 4 x PMF_VQ_TILE partial sums of its quad against one tile of 16 queries in registers (64 accumulators; with the running
// minima, the row's values and the staged queries well inside the 512 registers a 256-thread workgroup may use: no scratch);
// a tile of 128 would need 512 accumulators alone.  The quad is read once per tile -- nq / 16 times in all, of which all but the
// first come from L2: from 32 queries on the pass is bound by its 2 m n nq fp32 operations, not by the read of V.
//   m QP <= PMF_VQ_LDS floats: all queries are staged once, [m][QP] (64 x 128 fills the 32 KiB exactly);
//   otherwise: one tile at a time, [rows of a slab][16], slabs of PMF_VQ_LDS / 16 = 512 rows; the partial sums stay in
//   registers across the slabs of a quad, the slab is restaged behind a barrier (every loop around it is uniform).
// Arithmetic: fp32 from the difference (dist.py:61, dist.py:33): l2 sqrtf(sum (v - q)^2), l1 sum |v - q|; one running sum per
// (column, query) down the rows in ascending order.  No norm expansion.
// Argmin: a smaller distance wins, then the lower column (vq_better: a NaN never wins); columns c >= n are never offered.  Lane
// minima over its quads, the 64 lanes by the xor butterfly of sivm_wg_best, the four waves through LDS; one (distance, column) per
// workgroup and query into [wgs][QP].  k_vq_close (one workgroup per query) reduces them; the order is total, so the result does
// not depend on the partition.  No float atomics; two runs give the same bits.
// want_all: the same kernel also writes dist[q][c] (float64, leading dimension n) for q < nq, c < n, once; k_vq_argmin_rows takes
// per column the nearest query, lowest query on ties.
#pragma once
#include "pmf_colsweep.h"

enum { PMF_VQ_L2 = PMF_SIVM_L2, PMF_VQ_L1 = PMF_SIVM_L1 };
constexpr int PMF_VQ_MAX_Q = 128;     // queries of one call
constexpr int PMF_VQ_TILE = 16;       // queries whose partial sums a lane carries
constexpr int PMF_VQ_LDS = 8192;      // floats of staged queries (32 KiB)

struct VqArgs : ColsweepArgs {        // (pscore_in, pidx_in, nprev: not used; pscore_out, pidx_out: [wgs][QP])
  const float* Q;                     // [m][QP], zero beyond nq
  double* dall;                       // want_all: [nq][n]
  int nq, QP;
  int want_all;
};

// (distance, index): a smaller distance wins, then the lower index; a NaN never wins; offered: the candidate takes part at all
__device__ __forceinline__ void vq_better(float& s, int& i, float os, int oi, bool offered = true) {
  const bool b = offered && (os < s || (os == s && oi < i));
  s = b ? os : s;
  i = b ? oi : i;
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_vq_pass(const VqArgs a) {
  __shared__ __attribute__((aligned(16))) float qs[PMF_VQ_LDS];
  __shared__ float sb[4][PMF_VQ_TILE];
  __shared__ int ib[4][PMF_VQ_TILE];
  constexpr int T = PMF_VQ_TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = a.m, n = a.n, QP = a.QP;
  const int64_t np = a.np;
  const bool whole = (int64_t)m * QP <= PMF_VQ_LDS;    // all queries staged at once
  const int QL = whole ? QP : T;                       // queries per staged row
  const int SR = whole ? m : PMF_VQ_LDS / T;           // rows per slab
  int staged_t0 = -1, staged_r0 = -1;                  // what qs holds (uniform)

  for (int t0 = 0; t0 < QP; t0 += T) {
    float bd[T];
    int bi[T];
#pragma unroll
    for (int j = 0; j < T; ++j) { bd[j] = INFINITY; bi[j] = 0x7fffffff; }
    colsweep_quads_uniform(a, [&](const int c, const bool live) __attribute__((always_inline)) {   // (uniform trips: barriers inside)
      const float* vp = a.V + c;
      f32x4 acc[T];
#pragma unroll
      for (int j = 0; j < T; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int r0 = 0; r0 < m; r0 += SR) {
        const int want_t0 = whole ? 0 : t0;
        if (staged_t0 != want_t0 || staged_r0 != r0) {
          __syncthreads();                             // the readers of the previous image are through
          const int rows = min(SR, m - r0);
          for (int e = tid; e < rows * QL; e += 256) {
            const int r = e / QL, j = e - r * QL;
            qs[e] = a.Q[(int64_t)(r0 + r) * QP + want_t0 + j];
          }
          __syncthreads();
          staged_t0 = want_t0; staged_r0 = r0;
        }
        const float* qrow = qs + (t0 - want_t0);
        const int r1 = min(m, r0 + SR);
        auto step = [&](const f32x4 v, const int r) __attribute__((always_inline)) {
          const f32x4* qv = reinterpret_cast<const f32x4*>(qrow + (r - r0) * QL);
#pragma unroll
          for (int g = 0; g < T / 4; ++g) {
            const f32x4 q4 = qv[g];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
              const f32x4 d = v - q4[jj];
              if (METRIC == PMF_VQ_L2) {
                acc[4 * g + jj] += d * d;
              } else {
                acc[4 * g + jj] += __builtin_elementwise_abs(d);
              }
            }
          }
        };
        int r = r0;
        for (; r + 4 <= r1; r += 4) {
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 0) * np);
          const f32x4 v1 = *reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 1) * np);
          const f32x4 v2 = *reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 2) * np);
          const f32x4 v3 = *reinterpret_cast<const f32x4*>(vp + (int64_t)(r + 3) * np);
          step(v0, r + 0);                               // (the barriers keep a row's 16 staged queries from being read
          __builtin_amdgcn_sched_barrier(0);              // ahead of the row before it: 64 ds_read_b128 in flight cost the
          step(v1, r + 1);                               // l1 instantiation 485 registers)
          __builtin_amdgcn_sched_barrier(0);
          step(v2, r + 2);
          __builtin_amdgcn_sched_barrier(0);
          step(v3, r + 3);
          __builtin_amdgcn_sched_barrier(0);
        }
        for (; r < r1; ++r) step(*reinterpret_cast<const f32x4*>(vp + (int64_t)r * np), r);
      }
#pragma unroll
      for (int j = 0; j < T; ++j) {
        f32x4 dist = acc[j];
        if (METRIC == PMF_VQ_L2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) dist[e] = sqrtf(dist[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) vq_better(bd[j], bi[j], dist[e], c + e, live && c + e < n);
        if (live) {
          if (a.want_all && t0 + j < a.nq) {
            double* out = a.dall + (int64_t)(t0 + j) * n + c;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c + e < n) out[e] = (double)dist[e];
          }
        }
      }
    });
    // the workgroup's best per query of the tile: lanes, then waves
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
      for (int x = 1; x < 64; x <<= 1) {
        const float os = __shfl_xor(bd[j], x);
        const int oi = __shfl_xor(bi[j], x);
        vq_better(bd[j], bi[j], os, oi);
      }
      if (lane == 0) { sb[wave][j] = bd[j]; ib[wave][j] = bi[j]; }
    }
    __syncthreads();
    if (tid < T) {
      float s = sb[0][tid];
      int i = ib[0][tid];
      for (int w = 1; w < 4; ++w) vq_better(s, i, sb[w][tid], ib[w][tid]);
      a.pscore_out[(int64_t)blockIdx.x * QP + t0 + tid] = (double)s;
      a.pidx_out[(int64_t)blockIdx.x * QP + t0 + tid] = i;
    }
    __syncthreads();                                   // (sb, ib are rewritten by the next tile)
  }
}

// query blockIdx.x: the nearest column over the `count` workgroups' partials [count][QP]; an index outside [0, n) -- no
// comparable distance at all -- becomes column 0 with the distance NaN
__global__ __launch_bounds__(256) void k_vq_close(const double* __restrict__ ps, const int* __restrict__ pi, int count, int QP, int n,
                                                  int* __restrict__ idx_out, double* __restrict__ dist_out) {
  __shared__ float sb[4];
  __shared__ int ib[4];
  const int j = blockIdx.x;
  float s = INFINITY;
  int i = 0x7fffffff;
  for (int w = threadIdx.x; w < count; w += 256) vq_better(s, i, (float)ps[(int64_t)w * QP + j], pi[(int64_t)w * QP + j]);
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const float os = __shfl_xor(s, x);
    const int oi = __shfl_xor(i, x);
    vq_better(s, i, os, oi);
  }
  if ((threadIdx.x & 63) == 0) { sb[threadIdx.x >> 6] = s; ib[threadIdx.x >> 6] = i; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) vq_better(s, i, sb[w], ib[w]);
    const bool found = (unsigned)i < (unsigned)n;
    idx_out[j] = found ? i : 0;
    dist_out[j] = found ? (double)s : (double)NAN;
  }
}

// column c: the nearest of the nq queries in dall [nq][n], lowest query on ties; a NaN never wins (all NaN: query 0)
__global__ __launch_bounds__(256) void k_vq_argmin_rows(const double* __restrict__ dall, int nq, int n, int* __restrict__ idx_out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  double s = INFINITY;
  int i = 0x7fffffff;
  for (int q = 0; q < nq; ++q) {
    const double d = dall[(int64_t)q * n + c];
    if (d < s || (d == s && q < i)) { s = d; i = q; }
  }
  idx_out[c] = (unsigned)i < (unsigned)nq ? i : 0;
}
