// pmf_aa.h -- AA (pymf/aa.py): the W step, column i of W = the projection of W_hat[:, i] = (V pinv(H))[:, i] onto the convex
// hull of the data columns (aa.py:113-134), as column generation in data space -- the n x n Hessian V^T V of the reference's
// QPs is never formed.
//
// Per base i the state is a corral of at most min(m + 1, n) <= PMF_AA_MAX_CORRAL data columns with convex weights, the point
// X[:, i] = V beta_i and the residual R[:, i] = X[:, i] - W_hat[:, i] (both float32, [mp][KP]).  One round:
//   k_aa_price   G = R^T V on the fp32 MFMA, one pass over column panels of V; the k x n result is never written: the epilogue
//                keeps, per base, the smallest g_ij and the lowest column attaining it.  A workgroup owns a contiguous range of
//                64-column panels (panel_partition) and writes its partials [wg][KP]; no float atomics.
//   k_aa_master  one workgroup per base: reduces the partials (the lowest index wins ties), admits the priced column e when
//                g_min < beta^T g - tol, finds the affine minimiser on the corral in float64 -- (11^T + D^T D) u = 1,
//                a = u / sum u with D the corral columns minus W_hat[:, i]: positive definite exactly when the corral is
//                affinely independent, which the entering column's Cholesky pivot decides --, runs Wolfe's minor cycles (back
//                to the simplex along the line to the minimiser, dropping what reaches zero) and writes X, R and the weights.
// A base is finished when no column prices out, when the priced column is in the corral already, is affinely dependent on it
// or leaves it again at once (no progress possible in this precision), or when |R| is at float32 rounding level of W_hat.
// Pad columns (c >= n) never win; pad rows are zero in V and in the staged R.  Two runs give the same bits.
#pragma once
#include "pmf_dev.h"

constexpr int PMF_AA_MAX_CORRAL = 128;
constexpr int PMF_AA_MC = 128;          // rows of R staged in LDS at a time (k_aa_price)

template <int NT>
constexpr int aa_ldr() { return (16 * NT) % 32 == 16 ? 16 * NT : 16 * NT + 16; }   // row stride of the staged R: lanes l and l + 16 (next row) on different banks
template <int NT>
constexpr size_t aa_price_smem() { return (size_t)PMF_AA_MC * aa_ldr<NT>() * sizeof(float); }

struct AaPriceArgs {
  const float* V;          // [mp][np]
  const float* R;          // [mp][KP]
  float* pscore;           // [wgs][KP] partials of this launch
  int* pidx;
  int64_t np;
  int m, n, k;
  int npanels, panels_per_wg;
};

// (value, index): a smaller value wins, then the lower index
__device__ __forceinline__ void aa_better(float& s, int& i, float os, int oi) {
  if (os < s || (os == s && oi < i)) { s = os; i = oi; }
}

template <int NT>
__global__ __launch_bounds__(256) void k_aa_price(const AaPriceArgs a) {
  extern __shared__ float rs[];                 // [PMF_AA_MC][LDR]
  constexpr int KP = 16 * NT, LDR = aa_ldr<NT>();
  __shared__ float sbs[4][KP];
  __shared__ int sbi[4][KP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g4 = lane >> 4, l16 = lane & 15;
  const int64_t np = a.np;
  const int m4 = (a.m + 3) & ~3;
  const int nchunks = (m4 + PMF_AA_MC - 1) / PMF_AA_MC;
  const int p_begin = blockIdx.x * a.panels_per_wg;
  const int p_end = min(p_begin + a.panels_per_wg, a.npanels);

  float best[NT][4];
  int bidx[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) { best[t][r] = INFINITY; bidx[t][r] = 0x7fffffff; }

  // the four waves take the workgroup's panels in turn (wave w: p_begin + w, + 4, ...), every wave the whole contraction of
  // its panel: a lane reads 16 bytes of one row -- 4 adjacent columns, the B operands of 4 MFMAs --, 16 lanes 256 bytes
  for (int pb = p_begin; pb < p_end; pb += 4) {
    const int p = pb + wave;
    const bool live = p < p_end;
    f32x4 acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nchunks; ++ch) {
      const int r0 = ch * PMF_AA_MC;
      const int rows = min(PMF_AA_MC, m4 - r0);
      if (nchunks > 1 || pb == p_begin) {          // (R fits one chunk: staged once per launch)
        __syncthreads();
        for (int q = tid; q < rows * KP; q += 256) {
          const int rr = q / KP, j = q % KP;
          rs[rr * LDR + j] = (r0 + rr < a.m && j < a.k) ? a.R[(int64_t)(r0 + rr) * KP + j] : 0.f;
        }
        __syncthreads();
      }
      if (!live) continue;
      const float* vp = a.V + (int64_t)(r0 + g4) * np + 64 * (int64_t)p + 4 * l16;
#pragma unroll 4
      for (int kk = 0; kk < rows; kk += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(vp + (int64_t)kk * np);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float ra = rs[(kk + g4) * LDR + 16 * t + l16];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t][e] = mfma16(ra, v[e], acc[t][e]);
        }
      }
    }
    if (!live) continue;
    // ---- epilogue of the panel: columns in ascending order per lane, so a strict < keeps the lowest index ------------
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 64 * p + 4 * l16 + e;
      if (col >= a.n) continue;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float g = acc[t][e][r];
          if (g < best[t][r]) { best[t][r] = g; bidx[t][r] = col; }
        }
    }
  }
  // ---- the workgroup's best per base --------------------------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = best[t][r];
      int i = bidx[t][r];
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) {
        const float os = __shfl_xor(s, x);
        const int oi = __shfl_xor(i, x);
        aa_better(s, i, os, oi);
      }
      if (l16 == 0) { sbs[wave][16 * t + 4 * g4 + r] = s; sbi[wave][16 * t + 4 * g4 + r] = i; }
    }
  __syncthreads();
  if (tid < KP) {
    float s = sbs[0][tid];
    int i = sbi[0][tid];
    for (int w = 1; w < 4; ++w) aa_better(s, i, sbs[w][tid], sbi[w][tid]);
    a.pscore[(int64_t)blockIdx.x * KP + tid] = s;
    a.pidx[(int64_t)blockIdx.x * KP + tid] = i;
  }
}

// ---- the master step ------------------------------------------------------------------------------------------------------
struct AaMasterArgs {
  const float* V;          // [mp][np]
  const float* What;       // [mp][KP] W_hat
  float* X;                // [mp][KP] the current points V beta_i
  float* R;                // [mp][KP] X - W_hat
  const float* pscore;     // [nparts][KP] partials of the pricing pass in front
  const int* pidx;
  double* A;               // [k][LD][LD] Gram matrices of the corral columns minus W_hat[:, i], by slot
  int* cidx;               // [k][LD] data column of a slot, -1: free
  double* lam;             // [k][LD] its weight
  int* fin;                // [k]
  int* unfinished;         // [rounds + 1]
  int64_t np;
  int m, n, k, KP;
  int nparts, LD, round;
  int first;               // the first round: X = 0 and the corral is empty, the priced column is admitted without the test
  double tau, rho, piv;
};

static inline size_t aa_master_smem(int LD) { return ((size_t)LD * (LD + 1) + 6 * (size_t)LD) * sizeof(double) + (size_t)LD * sizeof(int); }

__device__ __forceinline__ double aa_wg_sum(double v, double* red) {   // the sum over the 256 threads, in every thread; fixed order
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) v += __shfl_xor(v, x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void k_aa_master(const AaMasterArgs a) {
  extern __shared__ double aa_lds[];
  const int LD = a.LD, LDM = LD + 1;
  double* M = aa_lds;                          // [LD][LDM]: the matrix 11^T + D^T D of the corral, then its Cholesky factor
  double* dinv = M + (size_t)LD * LDM;         // 1 / L_jj
  double* bv = dinv + LD;                      // right-hand side, then y
  double* uv = bv + LD;                        // u, then the affine minimiser
  double* lm = uv + LD;                        // the weights, by position in the list
  double* rowf = lm + LD;                      // the entering column's Gram row, by slot
  double* spare = rowf + LD;
  int* list = reinterpret_cast<int*>(spare + LD);   // the corral: slots in ascending order, the entering one last
  __shared__ double red[4];
  __shared__ float ps[4];
  __shared__ int pi[4];
  __shared__ int ctl[4];                       // [0] corral size, [1] minor cycles go on, [2] the entering column was dropped, [3] free slot
  const int base = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.fin[base]) return;
  const int64_t np = a.np;
  const int KP = a.KP;
  double* A = a.A + (size_t)base * LD * LD;
  int* cidx = a.cidx + (size_t)base * LD;
  double* lam = a.lam + (size_t)base * LD;

  // ---- the priced column: the argmin over the partials, the lowest index among equals --------------------------------
  float gs = INFINITY;
  int e = 0x7fffffff;
  for (int q = tid; q < a.nparts; q += 256) aa_better(gs, e, a.pscore[(int64_t)q * KP + base], a.pidx[(int64_t)q * KP + base]);
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const float os = __shfl_xor(gs, x);
    const int oi = __shfl_xor(e, x);
    aa_better(gs, e, os, oi);
  }
  if (lane == 0) { ps[wave] = gs; pi[wave] = e; }
  if (tid == 0) {                              // the corral as it stands, and the lowest free slot
    int s = 0, f = -1;
    for (int q = 0; q < LD; ++q) {
      if (cidx[q] >= 0) list[s++] = q;
      else if (f < 0) f = q;
    }
    ctl[0] = s; ctl[1] = 0; ctl[2] = 0; ctl[3] = f;
  }
  __syncthreads();
  gs = ps[0]; e = pi[0];
  for (int w = 1; w < 4; ++w) aa_better(gs, e, ps[w], pi[w]);
  int s = ctl[0];
  const int f = ctl[3];
  bool finished = (unsigned)e >= (unsigned)a.n || f < 0;
  if (!finished && !a.first) {
    double rr = 0.0, rx = 0.0, xx = 0.0, ww = 0.0, vv = 0.0;
    for (int r = tid; r < a.m; r += 256) {
      const double Rr = (double)a.R[(int64_t)r * KP + base], Xr = (double)a.X[(int64_t)r * KP + base];
      const double wr = (double)a.What[(int64_t)r * KP + base], vr = (double)a.V[(int64_t)r * np + e];
      rr = fma(Rr, Rr, rr); rx = fma(Rr, Xr, rx); xx = fma(Xr, Xr, xx); ww = fma(wr, wr, ww); vv = fma(vr, vr, vv);
    }
    rr = aa_wg_sum(rr, red); rx = aa_wg_sum(rx, red); xx = aa_wg_sum(xx, red); ww = aa_wg_sum(ww, red); vv = aa_wg_sum(vv, red);
    if (rr <= a.rho * a.rho * fmax(ww, xx)) finished = true;
    else if (!((double)gs < rx - a.tau * sqrt(rr) * sqrt(fmax(vv, xx)))) finished = true;
    else
      for (int q = 0; q < s; ++q)
        if (cidx[list[q]] == e) finished = true;
  }
  if (finished) {
    if (tid == 0) a.fin[base] = 1;
    return;
  }

  // ---- the entering column's Gram row: (v_e - w)^T (v_b - w) for every corral column b and for e itself ---------------
  if (tid == 0) list[s] = f;
  __syncthreads();
  for (int q = wave; q <= s; q += 4) {
    const int slot = list[q];
    const int cb = q == s ? e : cidx[slot];
    double d = 0.0;
    for (int r = lane; r < a.m; r += 64) {
      const double wr = (double)a.What[(int64_t)r * KP + base];
      d = fma((double)a.V[(int64_t)r * np + e] - wr, (double)a.V[(int64_t)r * np + cb] - wr, d);
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) d += __shfl_xor(d, x);
    if (lane == 0) { rowf[slot] = d; A[(size_t)f * LD + slot] = d; A[(size_t)slot * LD + f] = d; }
  }
  for (int q = tid; q <= s; q += 256) lm[q] = q == s ? 0.0 : lam[list[q]];
  s += 1;
  __syncthreads();

  bool first_solve = true, go_on = true, refused = false;
  while (go_on) {
    // M = 11^T + D^T D over the list (lower triangle)
    for (int q = tid; q < s * s; q += 256) {
      const int i = q / s, j = q % s;
      if (j > i) continue;
      const int si = list[i], sj = list[j];
      const double g = si == f ? rowf[sj] : sj == f ? rowf[si] : A[(size_t)si * LD + sj];
      M[(size_t)i * LDM + j] = g + 1.0;
    }
    // Cholesky: L_ij = M_ij / L_jj below the diagonal, M_jj keeps the pivot, dinv_j = 1 / L_jj
    double lastpiv = 0.0;
    for (int j = 0; j < s; ++j) {
      __syncthreads();
      const double d = M[(size_t)j * LDM + j];
      if (j == s - 1) lastpiv = d;
      const double rsq = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
      if (tid == 0) dinv[j] = rsq;
      for (int i = j + 1 + tid; i < s; i += 256) M[(size_t)i * LDM + j] *= rsq;
      __syncthreads();
      const int rem = s - j - 1;
      for (int q = tid; q < rem * rem; q += 256) {
        const int i = j + 1 + q / rem, c = j + 1 + q % rem;
        if (c <= i) M[(size_t)i * LDM + c] -= M[(size_t)i * LDM + j] * M[(size_t)c * LDM + j];
      }
    }
    __syncthreads();
    if (first_solve) {                         // affine independence of the entering column: its pivot against its diagonal entry
      first_solve = false;
      if (!(lastpiv > a.piv * (rowf[f] + 1.0))) { refused = true; break; }
    }
    // L y = 1, L^T u = y
    for (int q = tid; q < s; q += 256) bv[q] = 1.0;
    for (int j = 0; j < s; ++j) {
      __syncthreads();
      const double yj = bv[j] * dinv[j];
      for (int i = j + 1 + tid; i < s; i += 256) bv[i] -= M[(size_t)i * LDM + j] * yj;
      if (tid == 0) spare[j] = yj;
    }
    __syncthreads();
    for (int q = tid; q < s; q += 256) bv[q] = spare[q];
    for (int j = s - 1; j >= 0; --j) {
      __syncthreads();
      const double uj = bv[j] * dinv[j];
      for (int i = tid; i < j; i += 256) bv[i] -= M[(size_t)j * LDM + i] * uj;
      if (tid == 0) uv[j] = uj;
    }
    __syncthreads();
    if (tid == 0) {                            // the minor cycle's decision: a few hundred operations, one thread
      double us = 0.0;
      for (int q = 0; q < s; ++q) us += uv[q];
      bool inside = true;
      for (int q = 0; q < s; ++q) { uv[q] /= us; inside = inside && uv[q] > 0.0; }
      if (inside) {
        for (int q = 0; q < s; ++q) lm[q] = uv[q];
        ctl[1] = 0;
      } else {
        double theta = 1.0;
        for (int q = 0; q < s; ++q)
          if (!(uv[q] > 0.0)) theta = fmin(theta, lm[q] - uv[q] > 0.0 ? lm[q] / (lm[q] - uv[q]) : 0.0);
        theta = fmax(theta, 0.0);
        double mx = 1.0;
        for (int q = 0; q < s; ++q) { lm[q] = lm[q] + theta * (uv[q] - lm[q]); mx = fmax(mx, lm[q]); }
        int ndrop = 0, amin = -1;
        for (int q = 0; q < s; ++q)
          if (!(uv[q] > 0.0)) {
            if (amin < 0 || lm[q] < lm[amin]) amin = q;
            if (lm[q] <= 1e-15 * mx) ++ndrop;
          }
        int t = 0;
        for (int q = 0; q < s; ++q) {
          const bool drop = !(uv[q] > 0.0) && (ndrop > 0 ? lm[q] <= 1e-15 * mx : q == amin);
          if (drop) {
            if (list[q] == f) ctl[2] = 1;
            else { cidx[list[q]] = -1; lam[list[q]] = 0.0; }
          } else {
            list[t] = list[q]; lm[t] = fmax(lm[q], 0.0); ++t;
          }
        }
        ctl[0] = t;
        ctl[1] = 1;
      }
    }
    __syncthreads();
    go_on = ctl[1] != 0;
    if (go_on) s = ctl[0];
    __syncthreads();
  }
  if (refused) {                               // the corral stays as it was
    if (tid == 0) a.fin[base] = 1;
    return;
  }
  const bool gone = ctl[2] != 0;
  // ---- the new weights, X = V beta and R = X - W_hat ----------------------------------------------------------------------
  for (int q = tid; q < s; q += 256) {
    lam[list[q]] = lm[q];
    if (list[q] == f) cidx[f] = e;
  }
  __syncthreads();
  for (int r = tid; r < a.m; r += 256) {
    double x = 0.0;
    for (int q = 0; q < s; ++q) {
      const int slot = list[q];
      const int c = slot == f ? e : cidx[slot];
      x = fma(lm[q], (double)a.V[(int64_t)r * np + c], x);
    }
    a.X[(int64_t)r * KP + base] = (float)x;
    a.R[(int64_t)r * KP + base] = (float)(x - (double)a.What[(int64_t)r * KP + base]);
  }
  if (tid == 0) {
    if (gone) a.fin[base] = 1;
    else atomicAdd(a.unfinished + a.round, 1);
  }
}

// the state before the first round: X = 0, R = -W_hat, empty corrals
__global__ __launch_bounds__(256) void k_aa_init(const float* __restrict__ What, float* __restrict__ X, float* __restrict__ R, int64_t elems,
                                                 int* __restrict__ cidx, double* __restrict__ lam, int slots, int* __restrict__ fin, int k) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < elems) { X[i] = 0.f; R[i] = -What[i]; }
  if (i < slots) { cidx[i] = -1; lam[i] = 0.0; }
  if (i < k) fin[i] = 0;
}

// beta [k][n] float64 (zeroed by the caller) from the corrals
__global__ __launch_bounds__(256) void k_aa_beta(const int* __restrict__ cidx, const double* __restrict__ lam, int LD, int n, double* __restrict__ beta) {
  const int base = blockIdx.x;
  for (int q = threadIdx.x; q < LD; q += 256) {
    const int c = cidx[(size_t)base * LD + q];
    if (c >= 0 && c < n) beta[(size_t)base * n + c] = lam[(size_t)base * LD + q];
  }
}
