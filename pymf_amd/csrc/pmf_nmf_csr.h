// pmf_nmf_csr.h -- NMF (multiplicative update) on scipy.sparse CSR data, in gather form.  Semantics: dense NMF on V.toarray().
// Both half steps of nmf.py:122-132 are one operation on transposed operands,
//     X[r,:]  <-  X[r,:] * ( sum_{(r,c) in nz} v_rc Y[c,:] )  /  ( X[r,:] G + 1e-9 ),        G = Y^T Y  (k x k)
//   W step: rows of V,    X = W   (m x KP),  Y = H^T (n x KP),  G = H H^T;
//   H step: rows of V^T,  X = H^T (n x KP),  Y = W,             G = W^T W,
// so one kernel serves both, launched twice per iteration on the CSR arrays of V and of V^T (the host builds the second
// set once per upload, pmf_host_nmf_csr.h).  Nothing here is n-sized on chip and nothing scatters: no atomics on data, the
// entries of a row are added in stored order, the result is the same bits on every run.
#pragma once
#include "pmf_dev.h"

// waves per workgroup (they share one LDS image of G): eight, four at 128 bases, where the 36 S tiles, D and T of a wave
// take more than the 256 registers that eight waves leave each
__host__ __device__ constexpr int nmfsp_waves(int NT) { return NT == 8 ? 4 : 8; }
// LDS rows of G and of the waves' 16-row tiles are KP + 4 floats long: the four k-groups of an MFMA operand read (rows 4 apart)
// then fall 16 banks apart, and the 16 lanes of a fragment read (rows 1 apart, 16 bytes each) cover all 64 banks once
__host__ __device__ constexpr int nmfsp_ld(int KP) { return KP + 4; }
__host__ __device__ constexpr size_t nmfsp_smem_bytes(int NT) { return (size_t)(16 * NT + nmfsp_waves(NT) * 16) * nmfsp_ld(16 * NT) * sizeof(float); }

// Per 16-row block a wave
//   (1) gathers A = sum v Y[c,:]: KP / 4 lanes per row with four bases each (as k_csr_w_blocks, pmf_csr.h: one load for the
//       17 row pointers, one for the first 64 entries, entries beyond them straight from memory, wave-uniform trip counts),
//       Y through L2; X_b goes into the wave's LDS tile on the way and T = X_b * A stays in registers;
//   (2) forms D = X_b G on the fp32 MFMA (G in LDS);
//   (3) passes T through the tile into the accumulator layout and writes X_new = T / (D + 1e-9) -- multiply, then divide, as
//       nmf.py:124-126,130-132 order it;
//   (4) accumulates S += X_new^T X_new on the MFMA from the registers of (3) (tiles on and above the diagonal).
// A wave owns a contiguous range of blocks; the workgroup's waves add their S through LDS and write one KP x KP slab
// (row-major); the slabs are summed by k_reduce_slabs.  S is the G of the NEXT half step.
// Padded bases of X are 0 and stay 0 (T = 0, D = 0: 0 / 1e-9); padded and empty rows have A = 0, hence a zero row.
template <int NT>
__global__ __launch_bounds__(64 * nmfsp_waves(NT)) void k_nmf_sp_step(const int64_t* __restrict__ indptr,
                                                                  const int32_t* __restrict__ indices,
                                                                  const float* __restrict__ vals,
                                                                  int blk_per, int blk_extra,
                                                                  const float* __restrict__ Y,
                                                                  const float* __restrict__ G,
                                                                  float* __restrict__ X,
                                                                  float* __restrict__ slab) {
  constexpr int KP = 16 * NT, LD = nmfsp_ld(KP), NMFSP_WAVES = nmfsp_waves(NT);
  constexpr int LPR = KP / 4, RPI = 64 / LPR, NG = 16 / RPI;     // lanes per row, rows per group, groups per block
  constexpr int NS = NT * (NT + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* sG = sm;                                                // [KP][LD]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* sT = sG + KP * LD + wv * (16 * LD);                     // this wave's [16][LD]
  const int i = lane & 15, kq = lane >> 4;
  const int sub = lane / LPR, c4 = 4 * (lane % LPR);
  for (int q = tid; q < KP * LPR; q += 64 * NMFSP_WAVES)
    *reinterpret_cast<f32x4*>(sG + (q / LPR) * LD + 4 * (q % LPR)) = reinterpret_cast<const f32x4*>(G)[q];
  __syncthreads();

  const int gw = blockIdx.x * NMFSP_WAVES + wv;
  const int b0 = gw * blk_per + (gw < blk_extra ? gw : blk_extra);
  const int nb = blk_per + (gw < blk_extra ? 1 : 0);

  f32x4 S[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) S[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the row pointers of block b + 1 are requested while block b's rows are gathered, its first 64 entries while block b's
  // MFMAs execute (as k_snmf_csr_fused)
  auto load_ip = [&](int blk) -> long long {
    return (long long)indptr[(int64_t)blk * 16 + (lane < 17 ? lane : 16)];
  };
  auto base_of = [&](long long ipv) -> long long {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(ipv & 0xffffffffll), 0);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(ipv >> 32), 0);
    return (long long)(((unsigned long long)hi << 32) | lo);
  };
  long long ipv = nb > 0 ? load_ip(b0) : 0;
  long long a = base_of(ipv);
  int rel = (int)(ipv - a);                                       // lane r < 17: first entry of row r, block-relative
  int nzb = __builtin_amdgcn_readlane(rel, 16);
  int colv = 0;
  float valv = 0.f;
  if (lane < nzb) { colv = indices[a + lane]; valv = vals[a + lane]; }

  for (int b = 0; b < nb; ++b) {
    const int64_t r0 = (int64_t)(b0 + b) * 16;
    const bool more = b + 1 < nb;
    const long long ipv_n = more ? load_ip(b0 + b + 1) : 0;

    // ---- (1) A = sum v Y[c,:], T = X_b * A; X_b into the tile ----
    f32x4 T[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int row = g * RPI + sub;
      const f32x4 xv = *reinterpret_cast<const f32x4*>(X + (size_t)(r0 + row) * KP + c4);
      const int ea = __shfl(rel, row, 64), eb = __shfl(rel, row + 1, 64);
      const int cnt = eb - ea;
      int cmax = cnt;                                             // wave-uniform trip count: longest row of the group
#pragma unroll
      for (int o = 32; o >= LPR; o >>= 1) cmax = max(cmax, __shfl_xor(cmax, o, 64));
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int it = 0; it < cmax; it += 4) {                      // four gathers in flight, added in stored order
        f32x4 yr[4];
        float vv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = ea + it + u;
          int col = __shfl(colv, e & 63, 64);
          float val = __shfl(valv, e & 63, 64);
          const bool on = it + u < cnt;
          if (on && e >= 64) { col = indices[a + e]; val = vals[a + e]; }
          if (!on) { col = 0; val = 0.f; }
          vv[u] = val;
          yr[u] = *reinterpret_cast<const f32x4*>(Y + (size_t)col * KP + c4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += vv[u] * yr[u];         // duplicates add up, as in V.toarray()
      }
      *reinterpret_cast<f32x4*>(sT + row * LD + c4) = xv;
      T[g] = xv * acc;
    }
    // next block's first 64 entries: requested now, they land under the MFMAs below
    const long long a_n = base_of(ipv_n);
    const int rel_n = (int)(ipv_n - a_n);
    const int nzb_n = __builtin_amdgcn_readlane(rel_n, 16);
    int colv_n = 0;
    float valv_n = 0.f;
    if (more && lane < nzb_n) { colv_n = indices[a_n + lane]; valv_n = vals[a_n + lane]; }

    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // the wave's own tile writes are in place
    // ---- (2) D = X_b G: A[i = row][k = base], B[k = base][j = base'] ----
    f32x4 D[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) D[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f32x4 a4 = *reinterpret_cast<const f32x4*>(sT + i * LD + 16 * t + 4 * kq);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) D[nt] = mfma16(a4[e], sG[(16 * t + 4 * kq + e) * LD + 16 * nt + i], D[nt]);
    }
    // ---- (3) T into the accumulator layout (lane (i, kq), register j <-> row 4 kq + j, base 16 mt + i) ----
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // every lane has read X_b
#pragma unroll
    for (int g = 0; g < NG; ++g) *reinterpret_cast<f32x4*>(sT + (g * RPI + sub) * LD + c4) = T[g];
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float xn[NT][4];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xn[mt][j] = pmf_div(sT[(4 * kq + j) * LD + 16 * mt + i], D[mt][j] + PMF_EPS_DEN);
        X[(size_t)(r0 + 4 * kq + j) * KP + 16 * mt + i] = xn[mt][j];
      }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // ... before the next block's X_b overwrites the tile
    // ---- (4) S += X_new^T X_new: A[i = base][k = row], step j contracts the rows {4 q + j} ----
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int t = 0;
#pragma unroll
      for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int nt = mt; nt < NT; ++nt, ++t) S[t] = mfma16(xn[mt][j], xn[nt][j], S[t]);
    }
    ipv = ipv_n; a = a_n; rel = rel_n; nzb = nzb_n; colv = colv_n; valv = valv_n;
  }

  // ---- S: the waves' sums through LDS in wave order (the G image is dead now), wave 0 writes the slab row-major ----
  __syncthreads();
  f32x4* ex = reinterpret_cast<f32x4*>(sG);                       // NS KiB <= the G image
  static_assert((size_t)NS * 1024 <= (size_t)KP * LD * sizeof(float), "S exchange fits into the G image");
  for (int src = 1; src < NMFSP_WAVES; ++src) {
    if (wv == src) {
#pragma unroll
      for (int t = 0; t < NS; ++t) ex[t * 64 + lane] = S[t];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int t = 0; t < NS; ++t) S[t] += ex[t * 64 + lane];
    }
    __syncthreads();
  }
  if (wv == 0) {
    float* base = slab + (size_t)blockIdx.x * KP * KP;
    int t = 0;
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
      for (int nt = mt; nt < NT; ++nt, ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) base[(16 * mt + 4 * kq + j) * KP + 16 * nt + i] = S[t][j];
        if (nt > mt)
          *reinterpret_cast<f32x4*>(base + (16 * nt + i) * KP + 16 * mt + 4 * kq) = S[t];
      }
  }
}

// B = A^T for the row-major A [rows][cols] (lda) -> B [cols][rows] (ldb): H [KP][np] <-> H^T [np][KP], k x n sized
__global__ __launch_bounds__(256) void k_transpose_f32(const float* __restrict__ A, int64_t lda, int rows, int cols,
                                                       float* __restrict__ B, int64_t ldb) {
  __shared__ float t[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    const int r = by + j, c = bx + tx;
    t[j][tx] = (r < rows && c < cols) ? A[(int64_t)r * lda + c] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = bx + j, r = by + tx;
    if (c < cols && r < rows) B[(int64_t)c * ldb + r] = t[tx][j];
  }
}
