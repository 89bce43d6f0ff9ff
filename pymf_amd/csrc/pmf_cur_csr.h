// pmf_cur_csr.h -- CUR / CMD on CSR data (the reference's sparse branch of cur.py:84-120): the sampling norms, the gather of the
// chosen columns and rows and the middle product Cg^T data Rg^T over stored entries only.  No dense V exists on such a context.
//
// Arrays: the CSR image of V (indptr [mp + 1] int64, rows >= m empty; indices [nnz] int32, strictly ascending within a row;
// vals [nnz] float32) and the CSR image of V^T (tindptr [np + 1], tindices = row ids ascending within a column, tvals), both
// checked and built on the host before the upload (pmf_host_cur_csr.h).  A stored zero is a zero.
//
// k_cur_csr_sqnorms     out [mp + np] float64 = the row sums, then the column sums of (double) v * v: a team of 16 adjacent lanes
//                       owns one line (a CSR row, or a row of V^T), lane t takes entries t, t + 16, ... in order, the team's sums are
//                       combined by the xor tree 8, 4, 2, 1.  An empty line and a pad position give exactly 0.
// k_cur_csr_gather      the stored entries of column cid[j] into column j of the zeroed Cg [mp][cp], those of row rid[i] into row i
//                       of the zeroed Rg [rp][np] (the host zeroes both in stream order): one workgroup per slot, so a repeated
//                       index fills one slot per occurrence.
// k_cur_csr_mid<CP2>    part [chunk][b][a] float64 = sum over the entries (j, u) of chunk `chunk` of row rid[b] of
//                       u * sum over the entries (i, v) of column j of v * Cg[i][a]: grid = (rp, chunks), 256 threads, a chunk is
//                       PMF_CURSP_CHUNK entries of the row, so a fully dense row costs a workgroup no more than a short one's
//                       256 crossing columns.  The four waves share a crossing column: wave w loads entries 64 w + lane (+ 256 t)
//                       of it in one coalesced read and hands them round by v_readlane; lane l owns a = l (and l + 64: CP2 = 2) and
//                       reads the contiguous row i of Cg (256 or 512 bytes).  Products are exact in float64 (24 x 24 bits), the
//                       column's sum and u times it are rounded.  The waves' sums meet in LDS in wave order.
// k_cur_csr_mid_reduce  M [cp][rp] (a, b) = the sum of part [.][b][a] over the chunks in chunk order.
// No float atomics; the order of every sum is fixed by the launch shape, which follows from the data and the indices alone: two
// runs give the same bits.
#pragma once
#include "pmf_dev.h"

constexpr int PMF_CURSP_TEAM = 16;          // lanes per line of k_cur_csr_sqnorms
constexpr int PMF_CURSP_CHUNK = 256;        // entries of a selected row that one workgroup of k_cur_csr_mid takes

__global__ __launch_bounds__(256) void k_cur_csr_sqnorms(const int64_t* __restrict__ indptr, const float* __restrict__ vals, int64_t mp,
                                                         const int64_t* __restrict__ tindptr, const float* __restrict__ tvals, int64_t np,
                                                         double* __restrict__ out) {
  const int t = threadIdx.x & (PMF_CURSP_TEAM - 1);
  const int64_t line = (int64_t)blockIdx.x * (256 / PMF_CURSP_TEAM) + (threadIdx.x / PMF_CURSP_TEAM);
  const bool live = line < mp + np;               // (the xor tree below runs in every lane of the wave)
  const bool row = line < mp;
  double s = 0.0;
  if (live) {
    const int64_t* ip = row ? indptr + line : tindptr + (line - mp);
    const float* v = row ? vals : tvals;
    const int64_t hi = ip[1];
    for (int64_t e = ip[0] + t; e < hi; e += PMF_CURSP_TEAM) {
      const double x = (double)v[e];
      s += x * x;
    }
  }
#pragma unroll
  for (int d = PMF_CURSP_TEAM / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (live && t == 0) out[line] = s;
}

// grid = nc + nr workgroups: block j < nc scatters column cid[j], block nc + i row rid[i]; indices in range (the host checks)
__global__ __launch_bounds__(256) void k_cur_csr_gather(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                        const float* __restrict__ vals, const int64_t* __restrict__ tindptr,
                                                        const int32_t* __restrict__ tindices, const float* __restrict__ tvals,
                                                        const int* __restrict__ cid, int nc, int cp, const int* __restrict__ rid, int np,
                                                        float* __restrict__ Cg, float* __restrict__ Rg) {
  const int slot = (int)blockIdx.x;
  if (slot < nc) {
    const int col = cid[slot];
    const int64_t hi = tindptr[col + 1];
    for (int64_t e = tindptr[col] + threadIdx.x; e < hi; e += 256) Cg[(int64_t)tindices[e] * cp + slot] = tvals[e];
  } else {
    const int i = slot - nc, r = rid[i];
    const int64_t hi = indptr[r + 1];
    for (int64_t e = indptr[r] + threadIdx.x; e < hi; e += 256) Rg[(int64_t)i * np + indices[e]] = vals[e];
  }
}

template <int CP2>
__global__ __launch_bounds__(256) void k_cur_csr_mid(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                     const float* __restrict__ vals, const int64_t* __restrict__ tindptr,
                                                     const int32_t* __restrict__ tindices, const float* __restrict__ tvals,
                                                     const int* __restrict__ rid, const float* __restrict__ Cg, int rp,
                                                     double* __restrict__ part) {
  static_assert(CP2 == 1 || CP2 == 2, "Cg is one or two 64-wide tiles across");
  constexpr int CP = 64 * CP2;
  __shared__ double wsum[4][CP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = (int)blockIdx.x, chunk = (int)blockIdx.y;
  const int r = rid[b];
  const int64_t lo = indptr[r] + (int64_t)chunk * PMF_CURSP_CHUNK;
  const int64_t row_hi = indptr[r + 1];
  if (lo >= row_hi) return;                       // (uniform over the workgroup; the slot of `part` stays at the host's zero)
  const int64_t hi = lo + PMF_CURSP_CHUNK < row_hi ? lo + PMF_CURSP_CHUNK : row_hi;
  double acc[CP2];
#pragma unroll
  for (int h = 0; h < CP2; ++h) acc[h] = 0.0;
  for (int64_t e = lo; e < hi; ++e) {
    const int j = indices[e];                     // (uniform: every lane reads the same word)
    const double u = (double)vals[e];
    const int64_t c_hi = tindptr[j + 1];
    double t[CP2];
#pragma unroll
    for (int h = 0; h < CP2; ++h) t[h] = 0.0;
    for (int64_t f0 = tindptr[j] + 64 * wv; f0 < c_hi; f0 += 256) {
      const int cnt = (int)(c_hi - f0 < 64 ? c_hi - f0 : 64);
      const int my_i = lane < cnt ? tindices[f0 + lane] : 0;
      const float my_v = lane < cnt ? tvals[f0 + lane] : 0.f;
      for (int s = 0; s < cnt; ++s) {
        const int i = __builtin_amdgcn_readlane(my_i, s);
        const double v = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), s));
        const float* cr = Cg + (int64_t)i * CP + lane;
#pragma unroll
        for (int h = 0; h < CP2; ++h) t[h] += v * (double)cr[64 * h];
      }
    }
#pragma unroll
    for (int h = 0; h < CP2; ++h) acc[h] += u * t[h];
  }
#pragma unroll
  for (int h = 0; h < CP2; ++h) wsum[wv][64 * h + lane] = acc[h];
  __syncthreads();
  if (threadIdx.x < CP) {
    const int a = threadIdx.x;
    part[((int64_t)chunk * rp + b) * CP + a] = ((wsum[0][a] + wsum[1][a]) + wsum[2][a]) + wsum[3][a];
  }
}

// one thread per (a, b): grid = cp * rp / 256
__global__ __launch_bounds__(256) void k_cur_csr_mid_reduce(const double* __restrict__ part, int nchunks, int cp, int rp,
                                                            double* __restrict__ M) {
  const int q = (int)blockIdx.x * 256 + threadIdx.x;
  if (q >= cp * rp) return;
  const int b = q / cp, a = q % cp;               // (adjacent threads read adjacent words of part)
  double s = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) s += part[((int64_t)ch * rp + b) * cp + a];
  M[(int64_t)a * rp + b] = s;
}
