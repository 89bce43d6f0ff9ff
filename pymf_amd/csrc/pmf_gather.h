// pmf_gather.h -- k_gather_cols: the dense V of one context filled with chosen columns of another's, dst[r][j] = src[r][idx[j]]
// (pmf_set_v_gather_f32; SUB's column sample, pymf/sub.py:169).
//
// Both images are row-major and padded: src [.][snp], dst [mp][dnp], dnp a multiple of 64 floats, so every group of four
// adjacent destination columns starts on a 16-byte boundary of an allocation that starts on one.  A thread owns ONE such group and
// writes it with one 16-byte store per row; the threads of a workgroup form tx x ty (tx * ty = 256, tx = 16, 64 or 256 by the
// destination's width: a 64-column destination still fills its workgroups), tx adjacent groups along the row -- tx * 16
// contiguous bytes per row and store instruction -- and ty rows at a time.  The workgroup's slice of idx (4 tx entries) is read
// ONCE, each thread its four into registers, before the loop down the rows; the rows of a workgroup are PMF_GATHER_ROWS_IN_FLIGHT
// at a time so that the 4-byte reads at scattered columns of several source rows are in flight together.  A destination element is
// read as the 32-bit pattern it is and stored as such: NaN payloads, infinities and -0.0 pass unchanged.
// The pad (columns nsel .. dnp - 1, rows m .. mp - 1) is written as zeros, which is what the dense upload leaves there.
// Every destination element has exactly one writer: plain loads and vector stores, no atomics, no LDS, no barrier.
// IDENT (idx == nullptr, the whole copy): column j is column j, read with one 16-byte load where the group lies inside the
// source's n columns (snp is a multiple of 64 as well), so the copy runs at the rate of a plain one although the two leading
// dimensions may differ (the one-pass NMF kernels pad some widths further than the other families do).
// Bounds: the host has checked 0 <= idx[j] < n for every j < nsel before the launch; groups at or beyond dnp and rows at or
// beyond mp are never touched.
#pragma once

constexpr int PMF_GATHER_ROWS_IN_FLIGHT = 4;

struct GatherArgs {
  const uint32_t* src;     // [m][snp]
  uint32_t* dst;           // [mp][dnp]
  const int32_t* idx;      // [nsel]; not read by the IDENT form
  int64_t snp, dnp;
  int m, mp;               // valid / padded rows of dst (m of them exist in src)
  int n;                   // valid columns of src (IDENT: nsel == n)
  int nsel;                // valid columns of dst
  int tx_log2;             // 4, 6 or 8: threads along the row
  int rows_per_wg;         // a multiple of ty = 256 >> tx_log2
};

template <bool IDENT>
__global__ __launch_bounds__(256) void k_gather_cols(const GatherArgs a) {
  constexpr int R = PMF_GATHER_ROWS_IN_FLIGHT;
  const int tx = 1 << a.tx_log2, ty = 256 >> a.tx_log2;
  const int cx = threadIdx.x & (tx - 1), ry = threadIdx.x >> a.tx_log2;
  const int64_t c0 = ((int64_t)blockIdx.x * tx + cx) * 4;          // first of the thread's four destination columns
  if (c0 >= a.dnp) return;                                         // (dnp is a multiple of 4: the group is inside or outside)
  int sc[4];                                                       // their source columns, -1: pad
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t j = c0 + q;
    sc[q] = j < a.nsel ? (IDENT ? (int)j : a.idx[j]) : -1;
  }
  const bool vec = IDENT && c0 + 3 < a.n;                           // the whole copy: one 16-byte read serves the group
  const int r_lo = blockIdx.y * a.rows_per_wg;
  const int r_hi = min(r_lo + a.rows_per_wg, a.mp);
  for (int rb = r_lo + ry; rb < r_hi; rb += R * ty) {
    uint4 v[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int r = rb + u * ty;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      if (r < a.m && r < r_hi) {
        const uint32_t* s = a.src + (int64_t)r * a.snp;
        if (vec) {
          v[u] = *reinterpret_cast<const uint4*>(s + c0);
        } else {
          if (sc[0] >= 0) v[u].x = s[sc[0]];
          if (sc[1] >= 0) v[u].y = s[sc[1]];
          if (sc[2] >= 0) v[u].z = s[sc[2]];
          if (sc[3] >= 0) v[u].w = s[sc[3]];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int r = rb + u * ty;
      if (r < r_hi) *reinterpret_cast<uint4*>(a.dst + (int64_t)r * a.dnp + c0) = v[u];
    }
  }
}
