// pmf_cluster_csr.h -- Kmeans / Cmeans on CSR data.  The reference has no sparse clustering branch; the yardstick
// is its dense rule (kmeans.py:75-87, cmeans.py:71-86) on toarray().  No dense V exists on such a context: the H step sweeps the
// lines of the image of V^T (one line = one sample), the W step the lines of the image of V (one line = one data row).
//
// Arrays: the CSR image of V and of V^T as CUR / CMD keep them (pmf_cur_csr.h): indptr [lines_p + 1] int64 with the pad lines empty,
// indices [nnz] int32 strictly ascending within a line, vals [nnz] float32.  A stored zero is a zero.  W [mp][KP] float32 (dW);
// H lives transposed in float64, HT [np][LD], LD = 64 NH, NH = 1 (num_bases <= 64) or 2: a sample's memberships are one
// contiguous row for both kernels.  Columns >= num_bases and lines >= n of HT are zero and stay so.
//
// ccsr_line_sums<NH, T>        the gather of k_csr_proj_f64 / k_greedy_csr_pass as a function: the wave loads 64 entries of its
//                              stretch in one coalesced read and hands them round by v_readlane, four at a time; for an entry
//                              (r, v) lane l reads B[r][l] (and B[r][l + 64]), one contiguous read per entry and half, the four
//                              rows in flight together.  v * B is exact in float64 for a float32 B (24 x 24 bits) and rounds once
//                              in the fma for a float64 B.  Entry e of the stretch is added to accumulator e mod 4 in stored order;
//                              the caller combines (a0 + a1) + (a2 + a3).  Lanes >= cols read nothing and keep 0.
// k_cluster_csr_wnorm          wn[c] = |w_c|^2 in float64, one workgroup per column of W, an LDS tree.
// k_cluster_csr_assign<NH, A>  the H step.  256 threads; a workgroup takes lines_per_wg consecutive samples, wave w of it samples
//                              w, w + 4, ...; lane <-> centre.  d^2 = |v|^2 - 2 v.w_c + |w_c|^2 in float64, clamped at 0 (no
//                              translation by the row means: the three terms are float64, the products exact).  Lanes >= k are
//                              masked out of everything.  Kmeans: argmin over the lanes by the xor tree 32, 16, ..., 1, the lower
//                              index on ties; asg[j], the one-hot row of HT, the member counts and sum min d^2.  Cmeans:
//                              d = sqrt(d^2) + 1e-8, u_c = d_c^(-8/3) = 1 / cbrt(d_c)^8, H_c = u_c / sum_i u_i (the sum by the same
//                              tree), the row of HT, the row sums of H.  An empty line is at distance |w_c| from every centre and
//                              is handled like any other.  Pad lines are not swept.  A wave adds its lines in ascending order, the
//                              four waves meet in LDS as (s0 + s1) + (s2 + s3), the workgroup writes one partial row;
//                              k_cluster_totals (pmf_cluster.h) adds the partials in workgroup order.
// k_cluster_csr_den<NH, A>     the denominators alone, from asg (Kmeans) or HT (Cmeans), in the partition and order of the H step:
//                              for a W step that no pass preceded.
// k_cluster_csr_num<NH, A>     the W step's sums.  A line of the image of V is cut into chunks of PMF_CCSR_CHUNK entries (the host
//                              numbers them from indptr alone: chunk_off [mp + 1], chunk_row [chunks]); a wave owns one chunk, a
//                              workgroup four.  Cmeans: ccsr_line_sums against the rows of HT.  Kmeans: the wave gathers asg[j] of
//                              its 64 entries in one read, lane c adds v where asg[j] == c, one accumulator, stored order.
//                              part [chunk][LD] float64.
// k_cluster_csr_finish<A>      W[i][c] = (the chunk partials of row i in chunk order) / den: Kmeans only where the count is > 1,
//                              otherwise the column stays (kmeans.py:83-87); Cmeans den + 1e-8 (cmeans.py:83-86).  Rounded once to
//                              float32.  A row without entries has no chunk and gives 0.
// k_cluster_csr_widen, _ht     the error's float64 copy of W; HT <-> H [KP][np] float32 (to_h: rounded once).
// No atomics, no private segment; the order of every sum follows from indptr and the shape alone: two runs give the same bits.
// Open steps: several short lines per wave when num_bases <= 16 (a wave then idles 48 lanes); an LDS-staged W for few rows.
#pragma once
#include "pmf_cluster.h"

constexpr int PMF_CCSR_MIN_LINES = 64;      // samples a workgroup of k_cluster_csr_assign takes at least (16 per wave)
constexpr int PMF_CCSR_CHUNK = 512;         // entries of a data row that one wave of k_cluster_csr_num takes

template <int NH, typename T>
__device__ __forceinline__ void ccsr_line_sums(const int32_t* __restrict__ indices, const float* __restrict__ vals, int64_t lo, int64_t hi,
                                               const T* __restrict__ B, int ldb, int cols, int lane, double (&acc)[NH][4]) {
  bool on[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) on[h] = lane + 64 * h < cols;
  const T* Bl = B + lane;
  for (int64_t f0 = lo; f0 < hi; f0 += 64) {
    const int cnt = (int)(hi - f0 < 64 ? hi - f0 : 64);
    const int my_i = lane < cnt ? indices[f0 + lane] : 0;
    const int my_v = lane < cnt ? __float_as_int(vals[f0 + lane]) : 0;
    int s = 0;
    for (; s + 4 <= cnt; s += 4) {
      int ri[4];
      double v[4];
      T b[NH][4];
#pragma unroll
      for (int e = 0; e < 4; ++e) ri[e] = __builtin_amdgcn_readlane(my_i, s + e);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int h = 0; h < NH; ++h) b[h][e] = on[h] ? Bl[(int64_t)ri[e] * ldb + 64 * h] : (T)0;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + e));
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[h][e] = fma(v[e], (double)b[h][e], acc[h][e]);
    }
    if (s < cnt) {                                // the last one to three entries of the stretch (s is a multiple of 4)
      const int r0 = __builtin_amdgcn_readlane(my_i, s);
      const int r1 = __builtin_amdgcn_readlane(my_i, s + 1 < cnt ? s + 1 : s), r2 = __builtin_amdgcn_readlane(my_i, s + 2 < cnt ? s + 2 : s);
      const double v0 = (double)__int_as_float(__builtin_amdgcn_readlane(my_v, s));
      const double v1 = s + 1 < cnt ? (double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 1)) : 0.0;
      const double v2 = s + 2 < cnt ? (double)__int_as_float(__builtin_amdgcn_readlane(my_v, s + 2)) : 0.0;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const T b0 = on[h] ? Bl[(int64_t)r0 * ldb + 64 * h] : (T)0, b1 = on[h] ? Bl[(int64_t)r1 * ldb + 64 * h] : (T)0;
        const T b2 = on[h] ? Bl[(int64_t)r2 * ldb + 64 * h] : (T)0;
        acc[h][0] = fma(v0, (double)b0, acc[h][0]);
        if (s + 1 < cnt) acc[h][1] = fma(v1, (double)b1, acc[h][1]);
        if (s + 2 < cnt) acc[h][2] = fma(v2, (double)b2, acc[h][2]);
      }
    }
  }
}

// grid = KP workgroups; rows >= m of W are zero
__global__ __launch_bounds__(256) void k_cluster_csr_wnorm(const float* __restrict__ W, int64_t mp, int KP, double* __restrict__ wn) {
  __shared__ double part[256];
  const int j = blockIdx.x;
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < mp; r += 256) {
    const double w = (double)W[r * KP + j];
    s = fma(w, w, s);
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) wn[j] = part[0];
}

struct ClusterCsrArgs {
  const int64_t* indptr;       // [lines + 1 or more] the image of V^T: a line is a sample
  const int32_t* indices;      // row ids of W, < its row count (the host checks: csr_check)
  const float* vals;
  const float* W;              // [mp][KP]
  const double* vn2;           // [lines padded] |v_j|^2
  const double* wn;            // [KP] |w_c|^2
  double* HT;                  // [lines padded][64 NH]
  int* asg;                    // [lines padded] (Kmeans)
  double* pden;                // [wgs][64 NH]
  double* perr;                // [wgs][2]: sum min d^2 (Kmeans), 0
  int lines, lines_per_wg;     // samples; lines_per_wg a multiple of 4
  int k, KP;
};

// the waves' sums of a workgroup, one partial row per workgroup: (s0 + s1) + (s2 + s3)
template <int NH>
__device__ __forceinline__ void ccsr_wg_partials(const double (&den)[NH], double err, double* __restrict__ pden, double* __restrict__ perr) {
  constexpr int LD = 64 * NH;
  __shared__ double sden[4][LD];
  __shared__ double serr[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h < NH; ++h) sden[wv][lane + 64 * h] = den[h];
  if (lane == 0) serr[wv] = err;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < LD) pden[(int64_t)blockIdx.x * LD + t] = (sden[0][t] + sden[1][t]) + (sden[2][t] + sden[3][t]);
  if (t == 0) {
    perr[2 * (int64_t)blockIdx.x] = (serr[0] + serr[1]) + (serr[2] + serr[3]);
    perr[2 * (int64_t)blockIdx.x + 1] = 0.0;
  }
}

template <int NH, int ALGO>
__global__ __launch_bounds__(256) void k_cluster_csr_assign(const ClusterCsrArgs a) {
  static_assert(NH == 1 || NH == 2, "the centres are one or two 64-lane halves across");
  constexpr int LD = 64 * NH;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l_begin = (int)blockIdx.x * a.lines_per_wg;
  const int l_end = min(l_begin + a.lines_per_wg, a.lines);
  bool valid[NH];
  double wnr[NH], den[NH];
  double err = 0.0;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    valid[h] = lane + 64 * h < a.k;
    wnr[h] = valid[h] ? a.wn[lane + 64 * h] : 0.0;
    den[h] = 0.0;
  }
#pragma unroll 1
  for (int line = l_begin + wv; line < l_end; line += 4) {   // (uniform over the wave)
    double acc[NH][4];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[h][e] = 0.0;
    ccsr_line_sums<NH, float>(a.indices, a.vals, a.indptr[line], a.indptr[line + 1], a.W, a.KP, a.KP, lane, acc);
    const double v2 = a.vn2[line];
    double d2[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const double dot = (acc[h][0] + acc[h][1]) + (acc[h][2] + acc[h][3]);
      d2[h] = fmax(v2 - 2.0 * dot + wnr[h], 0.0);
    }
    double* hrow = a.HT + (int64_t)line * LD + lane;
    if (ALGO == PMF_CL_KMEANS) {
      double bd = 1e300;
      int bj = 0x7fffffff;
#pragma unroll
      for (int h = 0; h < NH; ++h)               // ascending index inside the lane: strict < keeps the lower one
        if (valid[h] && d2[h] < bd) { bd = d2[h]; bj = lane + 64 * h; }
#pragma unroll
      for (int x = 32; x >= 1; x >>= 1) {
        const double od = __shfl_xor(bd, x);
        const int oj = __shfl_xor(bj, x);
        if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
      }
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const double hv = lane + 64 * h == bj ? 1.0 : 0.0;
        hrow[64 * h] = hv;
        den[h] += hv;
      }
      if (lane == 0) a.asg[line] = bj;
      err += bd;
    } else {
      double u[NH];
      double us = 0.0;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const double t = cbrt(sqrt(d2[h]) + 1e-8);           // d^(1/3); d >= 1e-8: t^8 >= 1e-22, no overflow of 1 / t^8
        const double t2 = t * t, t4 = t2 * t2;
        u[h] = valid[h] ? 1.0 / (t4 * t4) : 0.0;
        us += u[h];
      }
#pragma unroll
      for (int x = 32; x >= 1; x >>= 1) us += __shfl_xor(us, x);
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const double hv = u[h] / us;
        hrow[64 * h] = hv;
        den[h] += hv;
      }
    }
  }
  ccsr_wg_partials<NH>(den, err, a.pden, a.perr);
}

template <int NH, int ALGO>
__global__ __launch_bounds__(256) void k_cluster_csr_den(const double* __restrict__ HT, const int* __restrict__ asg, int lines, int lines_per_wg,
                                                         double* __restrict__ pden, double* __restrict__ perr) {
  constexpr int LD = 64 * NH;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l_begin = (int)blockIdx.x * lines_per_wg;
  const int l_end = min(l_begin + lines_per_wg, lines);
  double den[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) den[h] = 0.0;
#pragma unroll 1
  for (int line = l_begin + wv; line < l_end; line += 4) {
    if (ALGO == PMF_CL_KMEANS) {
      const int bj = asg[line];
#pragma unroll
      for (int h = 0; h < NH; ++h) den[h] += lane + 64 * h == bj ? 1.0 : 0.0;
    } else {
#pragma unroll
      for (int h = 0; h < NH; ++h) den[h] += HT[(int64_t)line * LD + lane + 64 * h];
    }
  }
  ccsr_wg_partials<NH>(den, 0.0, pden, perr);
}

// grid = (chunks + 3) / 4 workgroups: wave w of workgroup b owns chunk 4 b + w
template <int NH, int ALGO>
__global__ __launch_bounds__(256) void k_cluster_csr_num(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                         const float* __restrict__ vals, const int* __restrict__ chunk_row,
                                                         const int* __restrict__ chunk_off, int nchunks, const double* __restrict__ HT,
                                                         const int* __restrict__ asg, double* __restrict__ part) {
  static_assert(NH == 1 || NH == 2, "the centres are one or two 64-lane halves across");
  constexpr int LD = 64 * NH;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = (int)blockIdx.x * 4 + wv;
  if (g >= nchunks) return;                       // (uniform over the wave; no barrier below)
  const int row = chunk_row[g];
  const int64_t lo = indptr[row] + (int64_t)(g - chunk_off[row]) * PMF_CCSR_CHUNK;
  const int64_t row_hi = indptr[row + 1];
  const int64_t hi = lo + PMF_CCSR_CHUNK < row_hi ? lo + PMF_CCSR_CHUNK : row_hi;
  double* out = part + (int64_t)g * LD + lane;
  if (ALGO == PMF_CL_CMEANS) {
    double acc[NH][4];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[h][e] = 0.0;
    ccsr_line_sums<NH, double>(indices, vals, lo, hi, HT, LD, LD, lane, acc);
#pragma unroll
    for (int h = 0; h < NH; ++h) out[64 * h] = (acc[h][0] + acc[h][1]) + (acc[h][2] + acc[h][3]);
  } else {
    double s[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) s[h] = 0.0;
    for (int64_t f0 = lo; f0 < hi; f0 += 64) {
      const int cnt = (int)(hi - f0 < 64 ? hi - f0 : 64);
      const int my_v = lane < cnt ? __float_as_int(vals[f0 + lane]) : 0;
      const int my_a = lane < cnt ? asg[indices[f0 + lane]] : -1;      // (column ids < n: the host checks)
      for (int e = 0; e < cnt; ++e) {
        const int c = __builtin_amdgcn_readlane(my_a, e);
        const double v = (double)__int_as_float(__builtin_amdgcn_readlane(my_v, e));
#pragma unroll
        for (int h = 0; h < NH; ++h) s[h] += lane + 64 * h == c ? v : 0.0;
      }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) out[64 * h] = s[h];
  }
}

// elems = m * KP; tot [ld] = the denominators
template <int ALGO>
__global__ __launch_bounds__(256) void k_cluster_csr_finish(const double* __restrict__ part, const int* __restrict__ chunk_off, int ld, int64_t elems,
                                                            int KP, int k, const double* __restrict__ tot, float* __restrict__ W) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  const int64_t i = e / KP;
  const int c = (int)(e % KP);
  if (c >= k) return;
  const double d = tot[c];
  if (ALGO == PMF_CL_KMEANS && !(d > 1.5)) return;
  const int g1 = chunk_off[i + 1];
  double s = 0.0;
  for (int g = chunk_off[i]; g < g1; ++g) s += part[(int64_t)g * ld + c];
  W[e] = (float)(ALGO == PMF_CL_KMEANS ? s / d : s / (d + 1e-8));
}

// Wd [mp][ld] float64 = W [mp][KP] float32 (columns >= k zero)
__global__ __launch_bounds__(256) void k_cluster_csr_widen(const float* __restrict__ W, int KP, int k, int ld, int64_t elems, double* __restrict__ Wd) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  const int64_t r = e / ld;
  const int j = (int)(e % ld);
  Wd[e] = j < k ? (double)W[r * KP + j] : 0.0;
}

// elems = np * ld; to_h: H[j][col] = (float) HT[col][j] for j < k; otherwise HT[col][j] = H[j][col] (columns >= k zero)
__global__ __launch_bounds__(256) void k_cluster_csr_ht(float* __restrict__ H, int np, int k, int ld, int64_t elems, double* __restrict__ HT, int to_h) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  const int64_t col = e / ld;
  const int j = (int)(e % ld);
  if (to_h) {
    if (j < k) H[(int64_t)j * np + col] = (float)HT[e];
  } else {
    HT[e] = j < k ? (double)H[(int64_t)j * np + col] : 0.0;
  }
}
