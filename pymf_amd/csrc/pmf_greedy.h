// pmf_greedy.h -- GREEDY (pymf/greedy.py, Civril and Magdon-Ismail): the num_bases columns of A that best reproduce the leading
// singular subspace, chosen one after the other.  The reference normalises and deflates the whole matrix in every round
// (greedy.py:122-158); here the data are read only.  With Q an orthonormal basis of the columns chosen so far
// and B' = (I - Q Q^T) B, B = (U S)[:, :num_bases], the reference's score of the original column v_j is
//   T_j = |B'^T v_j|^2 / (|v_j|^2 - |Q^T v_j|^2) .
//
// Wide A (rows <= cols): one round is
//   k_greedy_pass<NT>  [B' | Q]^T A on the fp32 MFMA, one pass over column panels of A; the staged operand Op [rows][128] holds
//                      B' in columns 0 .. c-1 and Q behind it, NT tiles of 16 columns cover the c + i columns in use.  The product
//                      is never written: the epilogue adds the squares of a column's entries over the tile rows (the numerator over
//                      rows < c, |Q^T v|^2 over the rest), forms the score and keeps the largest per workgroup, the lowest column
//                      among equals.  A column whose residual |v|^2 - |Q^T v|^2 is <= PMF_GREEDY_TAU32 |v|^2 scores 0, a chosen
//                      column -1, pad columns are not looked at.  Partials [wg], no float atomics.
//   k_greedy_step      one workgroup, float64: reduces the partials, appends the index, orthogonalises the chosen column against Q
//                      (classical Gram-Schmidt, twice), deflates B' by the new q and writes the float32 operand of the next round.
//                      k_greedy_step_csr is the same body with the chosen column read from a CSR line (pmf_greedy_csr.h).
// Tall A (rows > cols): k_greedy_gram runs all rounds in Gram space on G = A^T A (float64, cols x cols) and its eigenpairs:
// C' = B'^T A' starts as lambda_a e_a^T, the deflated Gram matrix is never formed -- its diagonal d and the rows in use follow
// from the pivoted-Cholesky vectors w_s = G'[:, i_s] / sqrt(G'[i_s, i_s]):  score_j = |C'[:, j]|^2 / d_j,
// w = (G[:, i] - sum_s w_s[i] w_s) / sqrt(d_i),  d -= w o w,  C' -= (C'[:, i] / sqrt(d_i)) w^T.  One workgroup.
// Two runs give the same bits.
#pragma once
#include "pmf_colsweep.h"   // sivm_better, sivm_wg_best, sivm_reduce_partials

constexpr int PMF_GREEDY_MAX_BASES = 64;
constexpr int PMF_GREEDY_OPW = 128;         // columns of the staged operand: c + i <= 2 * 64 - 1
constexpr int PMF_GREEDY_MC = 128;          // rows of the operand staged in LDS at a time
constexpr int PMF_GREEDY_MAX_ROWS = 2432;   // the short side (PMF_SVD_MAX_RANK): the chosen column lives in LDS in k_greedy_step
// a residual norm^2 at or below this multiple of the column's norm^2 is rounding: 512 unit roundoffs of the format the residual is
// formed in (fp32 MFMA sums of up to 2432 terms in the pass, float64 in Gram space)
constexpr double PMF_GREEDY_TAU32 = 512.0 * 5.9604644775390625e-8;
constexpr double PMF_GREEDY_TAU64 = 512.0 * 1.1102230246251565e-16;

template <int NT>
constexpr int greedy_ldr() { return (16 * NT) % 32 == 16 ? 16 * NT : 16 * NT + 16; }   // as aa_ldr: lanes l and l + 16 (next row) on different banks
template <int NT>
constexpr size_t greedy_pass_smem() { return (size_t)PMF_GREEDY_MC * greedy_ldr<NT>() * sizeof(float); }

struct GreedyPassArgs {
  const float* A;              // [rows padded][ld], zero padded
  const float* Op;             // [rows padded][PMF_GREEDY_OPW]
  const double* nrm2;          // [cols padded] |v_j|^2
  const unsigned char* taken;  // [cols padded] 1: chosen in an earlier round
  double* pscore;              // [wgs] partials of this launch
  int* pidx;
  int64_t ld;
  int m, n;                    // rows, columns of A
  int c;                       // columns of B'
  int npanels, panels_per_wg;
};

template <int NT>
__global__ __launch_bounds__(256) void k_greedy_pass(const GreedyPassArgs a) {
  extern __shared__ float gs_op[];              // [PMF_GREEDY_MC][LDR]
  constexpr int KP = 16 * NT, LDR = greedy_ldr<NT>();
  __shared__ double sb[4];
  __shared__ int ib[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g4 = lane >> 4, l16 = lane & 15;
  const int64_t ld = a.ld;
  const int m4 = (a.m + 3) & ~3;
  const int nchunks = (m4 + PMF_GREEDY_MC - 1) / PMF_GREEDY_MC;
  const int p_begin = blockIdx.x * a.panels_per_wg;
  const int p_end = min(p_begin + a.panels_per_wg, a.npanels);

  double best = -2.0;
  int bidx = 0x7fffffff;
  // the four waves take the workgroup's panels in turn, every wave the whole contraction of its panel (as k_aa_price)
  for (int pb = p_begin; pb < p_end; pb += 4) {
    const int p = pb + wave;
    const bool live = p < p_end;
    f32x4 acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nchunks; ++ch) {
      const int r0 = ch * PMF_GREEDY_MC;
      const int rows = min(PMF_GREEDY_MC, m4 - r0);
      if (nchunks > 1 || pb == p_begin) {          // (the operand fits one chunk: staged once per launch)
        __syncthreads();
        for (int q = tid; q < rows * KP; q += 256) {
          const int rr = q / KP, j = q % KP;
          gs_op[rr * LDR + j] = r0 + rr < a.m ? a.Op[(int64_t)(r0 + rr) * PMF_GREEDY_OPW + j] : 0.f;
        }
        __syncthreads();
      }
      if (!live) continue;
      const float* vp = a.A + (int64_t)(r0 + g4) * ld + 64 * (int64_t)p + 4 * l16;
#pragma unroll 4
      for (int kk = 0; kk < rows; kk += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(vp + (int64_t)kk * ld);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float ra = gs_op[(kk + g4) * LDR + 16 * t + l16];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t][e] = mfma16(ra, v[e], acc[t][e]);
        }
      }
    }
    if (!live) continue;
    // ---- epilogue of the panel: acc[t][e][r] is row 16 t + 4 g4 + r of the product, column 4 l16 + e of the panel ---------
    const int col0 = 64 * p + 4 * l16;
    const uchar4 tk = *reinterpret_cast<const uchar4*>(a.taken + col0);
    const unsigned char tke[4] = {tk.x, tk.y, tk.z, tk.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float num = 0.f, qs = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float g = acc[t][e][r];
          if (16 * t + 4 * g4 + r < a.c) num = fmaf(g, g, num);
          else qs = fmaf(g, g, qs);
        }
      num += __shfl_xor(num, 16); qs += __shfl_xor(qs, 16);
      num += __shfl_xor(num, 32); qs += __shfl_xor(qs, 32);
      const int col = col0 + e;
      if (col >= a.n) continue;
      const double v2 = a.nrm2[col];
      const double den = v2 - (double)qs;
      double s = (den > 0.0 && den > PMF_GREEDY_TAU32 * v2) ? (double)num / den : 0.0;
      if (tke[e]) s = -1.0;
      if (s > best) { best = s; bidx = col; }     // columns ascend per lane: a strict > keeps the lowest index
    }
  }
  sivm_wg_best(best, bidx, sb, ib);
  if (tid == 0) { a.pscore[blockIdx.x] = best; a.pidx[blockIdx.x] = bidx; }
}

// the sum over the 256 threads, in every thread; fixed order
__device__ __forceinline__ double greedy_wg_sum(double v, double* red) {
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) v += __shfl_xor(v, x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

struct GreedyStepArgs {
  const float* A;              // [rows padded][ld]
  const double* pscore;        // [nparts] partials of the pass in front
  const int* pidx;
  const double* nrm2;          // [cols padded]
  double* Bp;                  // [c][ldb] B', a column of it per row
  double* Q;                   // [nsel][ldb]
  float* Op;                   // [rows padded][PMF_GREEDY_OPW]
  int* select;                 // [nsel]
  unsigned char* taken;        // [cols padded]
  int64_t ld;
  int ldb;
  int m, n, c;
  int nparts, round;
  // the CSR form (k_greedy_step_csr): the image whose lines are the candidate columns stands in for A and ld
  const int64_t* indptr;
  const int32_t* indices;      // row ids < m (the host checks)
  const float* vals;
};

// CSR: the chosen column is a line of the image, scattered into the zeroed vector; everything behind the read is one text
template <bool CSR>
__device__ __forceinline__ void greedy_step_body(const GreedyStepArgs& a) {
  __shared__ double rv[PMF_GREEDY_MAX_ROWS];    // the chosen column, then its residual against Q
  __shared__ double dots[PMF_GREEDY_MAX_BASES];
  __shared__ double red[4];
  __shared__ double sb[4];
  __shared__ int ib[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = a.round, m = a.m, c = a.c, ldb = a.ldb;
  double best;
  int idx;
  sivm_reduce_partials(a.pscore, a.pidx, a.nparts, a.n, sb, ib, &best, &idx);
  if (tid == 0) { a.select[i] = idx; a.taken[idx] = 1; }
  if constexpr (CSR) {
    for (int r = tid; r < m; r += 256) rv[r] = 0.0;
    __syncthreads();
    const int64_t hi = a.indptr[idx + 1];
    for (int64_t e = a.indptr[idx] + tid; e < hi; e += 256) rv[a.indices[e]] = (double)a.vals[e];
  } else {
    for (int r = tid; r < m; r += 256) rv[r] = (double)a.A[(int64_t)r * a.ld + idx];
  }
  __syncthreads();
  // classical Gram-Schmidt against the i vectors of Q, twice: the dots of a sweep by waves, then one update
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int s = wave; s < i; s += 4) {
      const double* q = a.Q + (int64_t)s * ldb;
      double d = 0.0;
      for (int r = lane; r < m; r += 64) d = fma(q[r], rv[r], d);
#pragma unroll
      for (int x = 32; x >= 1; x >>= 1) d += __shfl_xor(d, x);
      if (lane == 0) dots[s] = d;
    }
    __syncthreads();
    for (int r = tid; r < m; r += 256) {
      double x = rv[r];
      for (int s = 0; s < i; ++s) x = fma(-dots[s], a.Q[(int64_t)s * ldb + r], x);
      rv[r] = x;
    }
    __syncthreads();
  }
  double nr2 = 0.0;
  for (int r = tid; r < m; r += 256) nr2 = fma(rv[r], rv[r], nr2);
  nr2 = greedy_wg_sum(nr2, red);
  const double v2 = a.nrm2[idx];
  // a residual at rounding level spans nothing new: q = 0, B' stays
  const double scale = (nr2 > 0.0 && nr2 > PMF_GREEDY_TAU32 * v2) ? 1.0 / sqrt(nr2) : 0.0;
  for (int r = tid; r < m; r += 256) {
    const double q = rv[r] * scale;
    rv[r] = q;
    a.Q[(int64_t)i * ldb + r] = q;
    if (c + i < PMF_GREEDY_OPW) a.Op[(int64_t)r * PMF_GREEDY_OPW + c + i] = (float)q;
  }
  __syncthreads();
  for (int s = wave; s < c; s += 4) {             // B'^T q
    const double* b = a.Bp + (int64_t)s * ldb;
    double d = 0.0;
    for (int r = lane; r < m; r += 64) d = fma(b[r], rv[r], d);
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) d += __shfl_xor(d, x);
    if (lane == 0) dots[s] = d;
  }
  __syncthreads();
  for (int e = tid; e < c * m; e += 256) {
    const int s = e / m, r = e % m;
    const double b = fma(-dots[s], rv[r], a.Bp[(int64_t)s * ldb + r]);
    a.Bp[(int64_t)s * ldb + r] = b;
    a.Op[(int64_t)r * PMF_GREEDY_OPW + s] = (float)b;
  }
}

__global__ __launch_bounds__(256) void k_greedy_step(const GreedyStepArgs a) { greedy_step_body<false>(a); }
__global__ __launch_bounds__(256) void k_greedy_step_csr(const GreedyStepArgs a) { greedy_step_body<true>(a); }

// The state in front of the first round.  QT [.][ldq]: eigenvectors of the short-side Gram matrix by rows, order / sv: the c kept
// ones in descending order and sqrt of their eigenvalues.  wide: B'_a = sv_a e_a (Bp [c][ldb], Op columns 0 .. c-1, the rest of Op
// zero);  otherwise C'_a = sv_a^2 e_a (Bp [c][ldb]) and d = diag G.  taken = 0 either way.
__global__ __launch_bounds__(256) void k_greedy_init(const double* __restrict__ QT, int ldq, const int* __restrict__ order,
                                                     const double* __restrict__ sv, int c, int q, int ldb, int wide, double* __restrict__ Bp,
                                                     float* __restrict__ Op, int64_t op_elems, const double* __restrict__ G, double* __restrict__ d,
                                                     unsigned char* __restrict__ taken, int ntaken) {
  const int64_t total = max(max((int64_t)c * ldb, op_elems), (int64_t)ntaken);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    if (e < (int64_t)c * ldb) {
      const int s = (int)(e / ldb), r = (int)(e % ldb);
      const double f = wide ? sv[s] : sv[s] * sv[s];
      Bp[e] = r < q ? f * QT[(int64_t)order[s] * ldq + r] : 0.0;
    }
    if (wide && e < op_elems) {
      const int64_t r = e / PMF_GREEDY_OPW;
      const int s = (int)(e % PMF_GREEDY_OPW);
      Op[e] = (s < c && r < q) ? (float)(sv[s] * QT[(int64_t)order[s] * ldq + r]) : 0.f;
    }
    if (e < ntaken) {
      taken[e] = 0;
      if (!wide) d[e] = e < q ? G[e * ldq + e] : 0.0;
    }
  }
}

// (score, index) best over the 1024 threads of the workgroup, in every thread
__device__ __forceinline__ void greedy_wg_best1024(double& s, int& i, double* sb, int* ib) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const double os = __shfl_xor(s, x);
    const int oi = __shfl_xor(i, x);
    sivm_better(s, i, os, oi);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sb[threadIdx.x >> 6] = s; ib[threadIdx.x >> 6] = i; }
  __syncthreads();
  s = sb[0]; i = ib[0];
  for (int w = 1; w < 16; ++w) sivm_better(s, i, sb[w], ib[w]);
}

// All rounds of the selection in Gram space.  G [.][ld] = A^T A, Cp [c][ld] = C' (k_greedy_init), d [ld] = diag G', Wm [nsel][ld]
// the pivoted-Cholesky vectors, n = the columns of A.  One workgroup of 1024 threads, a thread owns columns tid, tid + 1024, ...
__global__ __launch_bounds__(1024) void k_greedy_gram(const double* __restrict__ G, int ld, int n, int c, int nsel, double* __restrict__ Cp,
                                                      double* __restrict__ d, double* __restrict__ Wm, int* __restrict__ select,
                                                      unsigned char* __restrict__ taken) {
  __shared__ double sb[16];
  __shared__ int ib[16];
  __shared__ double ci[PMF_GREEDY_MAX_BASES], wi[PMF_GREEDY_MAX_BASES];
  const int tid = threadIdx.x;
  for (int i = 0; i < nsel; ++i) {
    double best = -2.0;
    int idx = 0x7fffffff;
    for (int j = tid; j < n; j += 1024) {
      const double dj = d[j];
      double s = 0.0;
      if (taken[j]) s = -1.0;
      else if (dj > 0.0 && dj > PMF_GREEDY_TAU64 * G[(int64_t)j * ld + j]) {
        double t = 0.0;
        for (int a = 0; a < c; ++a) { const double x = Cp[(int64_t)a * ld + j]; t = fma(x, x, t); }
        s = t / dj;
      }
      if (s > best) { best = s; idx = j; }
    }
    greedy_wg_best1024(best, idx, sb, ib);
    if ((unsigned)idx >= (unsigned)n) idx = 0;
    const double di = d[idx];
    const bool live = di > 0.0 && di > PMF_GREEDY_TAU64 * G[(int64_t)idx * ld + idx];
    if (tid < c) ci[tid] = Cp[(int64_t)tid * ld + idx];
    if (tid >= 64 && tid < 64 + i) wi[tid - 64] = Wm[(int64_t)(tid - 64) * ld + idx];
    __syncthreads();                              // (column idx is read in its state before this round by every thread)
    if (tid == 0) { select[i] = idx; taken[idx] = 1; }
    const double rs = live ? 1.0 / sqrt(di) : 0.0;
    for (int j = tid; j < n; j += 1024) {
      double w = 0.0;
      if (live) {
        w = G[(int64_t)j * ld + idx];
        for (int s = 0; s < i; ++s) w = fma(-wi[s], Wm[(int64_t)s * ld + j], w);
        w *= rs;
        d[j] = fma(-w, w, d[j]);
        for (int a = 0; a < c; ++a) Cp[(int64_t)a * ld + j] = fma(-(ci[a] * rs), w, Cp[(int64_t)a * ld + j]);
      }
      Wm[(int64_t)i * ld + j] = w;
    }
    __syncthreads();
  }
}

// O [cols][ldo] = the transpose of V [rows][ldv] (both zero padded to multiples of 64): 64 x 64 tiles through LDS;
// grid = (rows / 64, cols / 64)
__global__ __launch_bounds__(256) void k_greedy_transpose(const float* __restrict__ V, int64_t ldv, float* __restrict__ O, int64_t ldo) {
  __shared__ float tile[64][65];
  const int64_t r0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) tile[r][tx] = V[(r0 + r) * ldv + c0 + tx];
  __syncthreads();
  for (int r = ty; r < 64; r += 4) O[(c0 + r) * ldo + r0 + tx] = tile[tx][r];
}

// MT [mp][KP] float32 = (P W^T)^T: row r, column j = sum_q P[j][q] W[r][q] in float64, rounded once; padding zero
__global__ __launch_bounds__(256) void k_greedy_pinv_t(const float* __restrict__ W, const double* __restrict__ P, int64_t m, int k, int KP,
                                                       int64_t elems, float* __restrict__ MT) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  const int64_t r = e / KP;
  const int j = (int)(e % KP);
  double s = 0.0;
  if (r < m && j < k)
    for (int q = 0; q < k; ++q) s = fma(P[(int64_t)j * k + q], (double)W[r * KP + q], s);
  MT[e] = (float)s;
}
