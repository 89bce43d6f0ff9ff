// pmf_cluster.h -- Kmeans / Cmeans (pymf/kmeans.py, pymf/cmeans.py): one pass over V per iteration, spread over COLUMN panels.
//
// Clustering data are wide (many samples = columns, few dimensions = rows), so a workgroup owns a contiguous range of
// 64-column panels of V [mp][np] (a wave: 16 columns of each) and, per iteration (k_cluster_pass),
//   A  for each of its panels: P = W^T V_panel on the fp32 MFMA (64-row tiles of W staged in LDS, V read from global, a panel
//      row being one contiguous segment), ||v_c||^2 on the way; d^2 = ||w_j||^2 - 2 P_jc + ||v_c||^2 clamped at 0 (float64).
//      The expansion cancels where d^2 << ||v||^2, so w and v are both taken relative to mu = the row means of V (fp32,
//      k_cluster_rowmean; a distance does not change under a translation): subtracted from W as it is staged, from V as it
//      is loaded, and ||w_j - mu||^2 is what k_cluster_wnorm forms.  Data far from the origin then cost no digits;
//      Kmeans: argmin_j (lowest index on ties) -> assigned, one-hot H column; Cmeans: H_jc = d_j^-e / sum_i d_i^-e with
//      d = sqrt(d^2) + 1e-8, e = 2 / (m - 1) = 8/3 (cmeans.py:73-81); denominators (member counts / row sums of H) and
//      Kmeans' error sum_c min_j d^2 accumulated in float64;
//   B  for each 64-row tile: Num = V_tile H_range^T on the MFMA over ALL its columns, written once into the workgroup's slab.
// k_cluster_totals / k_cluster_finish add the slabs up in a fixed order in float64 and divide (kmeans.py:83-87,
// cmeans.py:83-86): no float atomics anywhere, two runs give the same bits.  assign = 0 skips the MFMA of A and takes H (Cmeans)
// or the assignment (Kmeans) as it is: the sums for an update_w() that no pass preceded.  B and the sums keep the untranslated V.
#pragma once
#include "pmf_dev.h"

enum { PMF_CL_KMEANS = 0, PMF_CL_CMEANS = 1 };
constexpr int PMF_CL_MAX_WGS = 1024;

struct ClusterArgs {
  const float* V;       // [mp][np]
  const float* W;       // [mp][KP]
  const float* mu;      // [mp] row means of V
  float* H;             // [KP][np]
  int* asg;             // [np] (Kmeans; -1 in the pad columns)
  const double* wn;     // [KP] ||w_j - mu||^2
  float* num;           // [wgs][mp][KP]
  double* den;          // [wgs][KP]
  double* err;          // [wgs][2]: sum_c min_j d^2, sum_c ||v_c - mu||^2 (Kmeans)
  int64_t mp;
  int np, n, k, npanels, panels_per_wg, assign;
  float expo;           // Cmeans: 2 / (m - 1)
};

// mu[r] = mean over the n samples of V[r][.] (pad columns are zero): float64 sum in a fixed order, one workgroup per row
__global__ __launch_bounds__(256) void k_cluster_rowmean(const float* __restrict__ V, int64_t np, int n, float* __restrict__ mu) {
  __shared__ double part[256];
  const float* row = V + (int64_t)blockIdx.x * np;
  double s = 0.0;
  for (int64_t q = threadIdx.x; q < np / 4; q += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
    s += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) mu[blockIdx.x] = (float)(part[0] / (double)n);
}

// ||w_j - mu||^2 in float64 (the difference in fp32, as k_cluster_pass stages it), one workgroup per basis
__global__ __launch_bounds__(256) void k_cluster_wnorm(const float* __restrict__ W, const float* __restrict__ mu, int64_t mp, int KP,
                                                       double* __restrict__ wn) {
  __shared__ double part[256];
  const int j = blockIdx.x;
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < mp; r += 256) {
    const double w = (double)(W[r * KP + j] - mu[r]);
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

template <int NT, int ALGO>
__global__ __launch_bounds__(256) void k_cluster_pass(const ClusterArgs a) {
  constexpr int KP = 16 * NT;
  constexpr int LW = KP == 16 ? 16 : KP + 16;   // row stride = 16 mod 64 floats: the 4 rows of an A fragment on 4 x 16 different banks
  __shared__ float wt[64 * LW];
  __shared__ float smu[64];
  __shared__ double sden[4][KP];
  __shared__ double serr[4][2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lg = lane >> 4;
  const int p0 = blockIdx.x * a.panels_per_wg, p1 = min(p0 + a.panels_per_wg, a.npanels);
  const int ntiles = (int)(a.mp / 64);
  const int64_t np = a.np;

  double den[NT][4], wnr[NT][4];
  double err = 0.0, vsum = 0.0;
#pragma unroll
  for (int jt = 0; jt < NT; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      den[jt][r] = 0.0;
      wnr[jt][r] = a.assign ? a.wn[jt * 16 + 4 * lg + r] : 0.0;
    }

  // ---- A: assignment / memberships of every panel, denominators, error ------------------------------------------------
  for (int p = p0; p < p1; ++p) {
    const int c = p * 64 + wave * 16 + lc;       // this lane's column (all four lane groups of a wave: the same 16)
    const bool valid = c < a.n;
    float hv[NT][4];
    if (a.assign) {
      f32x4 acc[NT];
#pragma unroll
      for (int jt = 0; jt < NT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
      float vn = 0.f;
      for (int rt = 0; rt < ntiles; ++rt) {
        if (ntiles > 1 || p == p0) {             // (a W of one tile is staged once per workgroup)
          __syncthreads();
          const float* wsrc = a.W + (int64_t)rt * 64 * KP;
          const float* msrc = a.mu + (int64_t)rt * 64;
          for (int q = tid; q < 64 * (KP / 4); q += 256) {
            const int row = q / (KP / 4), ch = q % (KP / 4);
            const float mr = msrc[row];
            f32x4 w = *reinterpret_cast<const f32x4*>(wsrc + row * KP + 4 * ch);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] -= mr;
            *reinterpret_cast<f32x4*>(wt + row * LW + 4 * ch) = w;
          }
          if (tid < 64) smu[tid] = msrc[tid];
          __syncthreads();
        }
        const float* vp = a.V + ((int64_t)rt * 64 + lg) * np + c;
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {           // rows 4 s + lg: A = W[row][16 jt + lc], B = V[row][c]
          const float v = vp[(int64_t)(4 * s) * np] - smu[4 * s + lg];
          vn = fmaf(v, v, vn);
          const float* wl = wt + (4 * s + lg) * LW + lc;
#pragma unroll
          for (int jt = 0; jt < NT; ++jt) acc[jt] = mfma16(wl[16 * jt], v, acc[jt]);
        }
      }
      vn += __shfl_xor(vn, 16);
      vn += __shfl_xor(vn, 32);
      // acc[jt][r] = P[j = 16 jt + 4 lg + r][c]
      double d2[NT][4];
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          d2[jt][r] = fmax(wnr[jt][r] - 2.0 * (double)acc[jt][r] + (double)vn, 0.0);
      if (ALGO == PMF_CL_KMEANS) {
        double bd = 1e300;
        int bj = KP;
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {          // ascending j inside the lane: strict < keeps the lowest index
            const int j = jt * 16 + 4 * lg + r;
            if (j < a.k && d2[jt][r] < bd) { bd = d2[jt][r]; bj = j; }
          }
#pragma unroll
        for (int x = 16; x <= 32; x <<= 1) {
          const double od = __shfl_xor(bd, x);
          const int oj = __shfl_xor(bj, x);
          if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
        }
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
          for (int r = 0; r < 4; ++r) hv[jt][r] = (valid && jt * 16 + 4 * lg + r == bj) ? 1.f : 0.f;
        if (lg == 0) {
          a.asg[c] = valid ? bj : -1;
          if (valid) { err += bd; vsum += (double)vn; }
        }
      } else {
        float df[NT][4];
        float dmin = 3.0e38f;
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            df[jt][r] = (float)sqrt(d2[jt][r]) + 1e-8f;
            if (jt * 16 + 4 * lg + r < a.k) dmin = fminf(dmin, df[jt][r]);
          }
        dmin = fminf(dmin, __shfl_xor(dmin, 16));
        dmin = fminf(dmin, __shfl_xor(dmin, 32));
        float usum = 0.f;
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {          // (d_min / d_j)^e <= 1: no overflow whatever the scale of the data
            const float u = (jt * 16 + 4 * lg + r < a.k) ? exp2f(a.expo * log2f(dmin / df[jt][r])) : 0.f;
            hv[jt][r] = u;
            usum += u;
          }
        usum += __shfl_xor(usum, 16);
        usum += __shfl_xor(usum, 32);
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
          for (int r = 0; r < 4; ++r) hv[jt][r] = valid ? hv[jt][r] / usum : 0.f;
      }
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) a.H[(int64_t)(jt * 16 + 4 * lg + r) * np + c] = hv[jt][r];
    } else {
      const int as = ALGO == PMF_CL_KMEANS ? a.asg[c] : -1;
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = jt * 16 + 4 * lg + r;
          if (ALGO == PMF_CL_KMEANS) hv[jt][r] = (valid && as == j) ? 1.f : 0.f;
          else hv[jt][r] = (valid && j < a.k) ? a.H[(int64_t)j * np + c] : 0.f;
        }
    }
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) den[jt][r] += (double)hv[jt][r];
  }

  // the 16 columns of a wave, then the 4 waves: fixed order
#pragma unroll
  for (int jt = 0; jt < NT; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double s = den[jt][r];
#pragma unroll
      for (int x = 1; x <= 8; x <<= 1) s += __shfl_xor(s, x);
      if (lc == 0) sden[wave][jt * 16 + 4 * lg + r] = s;
    }
#pragma unroll
  for (int x = 1; x <= 8; x <<= 1) {
    err += __shfl_xor(err, x);
    vsum += __shfl_xor(vsum, x);
  }
  if (lane == 0) { serr[wave][0] = err; serr[wave][1] = vsum; }
  __syncthreads();                               // (also: this workgroup's H / asg writes are visible to all its waves)
  if (tid < KP) a.den[(int64_t)blockIdx.x * KP + tid] = (sden[0][tid] + sden[1][tid]) + (sden[2][tid] + sden[3][tid]);
  if (tid < 2) a.err[2 * (int64_t)blockIdx.x + tid] = (serr[0][tid] + serr[1][tid]) + (serr[2][tid] + serr[3][tid]);

  // ---- B: Num[row][j] = sum_c V[row][c] H[j][c] over the workgroup's columns ------------------------------------------
  // A = V[r0 + lc][c0 + 4 lg + e], B = H[16 jt + lc][c0 + 4 lg + e]: one 16-byte read feeds 4 MFMAs (k order is free)
  float* slab = a.num + (int64_t)blockIdx.x * a.mp * KP;
  for (int rt = 0; rt < ntiles; ++rt) {
    const int64_t r0 = (int64_t)rt * 64 + wave * 16;
    f32x4 acc[NT];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = p0 * 64; c0 < p1 * 64; c0 += 16) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(a.V + (r0 + lc) * np + c0 + 4 * lg);
      if (ALGO == PMF_CL_KMEANS) {
        const int4 as = *reinterpret_cast<const int4*>(a.asg + c0 + 4 * lg);
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) {
          const int j = jt * 16 + lc;
          acc[jt] = mfma16(va[0], as.x == j ? 1.f : 0.f, acc[jt]);
          acc[jt] = mfma16(va[1], as.y == j ? 1.f : 0.f, acc[jt]);
          acc[jt] = mfma16(va[2], as.z == j ? 1.f : 0.f, acc[jt]);
          acc[jt] = mfma16(va[3], as.w == j ? 1.f : 0.f, acc[jt]);
        }
      } else {
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) {
          const f32x4 hb = *reinterpret_cast<const f32x4*>(a.H + (int64_t)(jt * 16 + lc) * np + c0 + 4 * lg);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[jt] = mfma16(va[e], hb[e], acc[jt]);
        }
      }
    }
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) slab[(r0 + 4 * lg + r) * KP + jt * 16 + lc] = acc[jt][r];
  }
}

// tot[0 .. KP) = denominators, tot[KP] = sum_c min_j d^2, tot[KP + 1] = sum_c ||v_c - mu||^2: the workgroups' partials in order
__global__ __launch_bounds__(256) void k_cluster_totals(const double* __restrict__ den, const double* __restrict__ err, int wgs, int KP,
                                                        double* __restrict__ tot) {
  const int t = threadIdx.x;
  if (t < KP) {
    double s = 0.0;
    for (int g = 0; g < wgs; ++g) s += den[(int64_t)g * KP + t];
    tot[t] = s;
  } else if (t < KP + 2) {
    double s = 0.0;
    for (int g = 0; g < wgs; ++g) s += err[2 * (int64_t)g + (t - KP)];
    tot[t] = s;
  }
}

// W = Num / Den.  Kmeans: only centres with more than one member (kmeans.py:83-87); Cmeans: Den + 1e-8 (cmeans.py:83-86)
template <int ALGO>
__global__ __launch_bounds__(256) void k_cluster_finish(const float* __restrict__ num, int wgs, int64_t elems, int KP,
                                                        const double* __restrict__ tot, float* __restrict__ W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= elems) return;
  const double d = tot[i % KP];
  if (ALGO == PMF_CL_KMEANS && !(d > 1.5)) return;
  double s = 0.0;
  for (int g = 0; g < wgs; ++g) s += (double)num[(int64_t)g * elems + i];
  W[i] = (float)(ALGO == PMF_CL_KMEANS ? s / d : s / (d + 1e-8));
}
