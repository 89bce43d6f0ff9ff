// pmf_gsat.h -- SIVM_GSAT (pymf/sivm_gsat.py:82-125): the online, swap-based simplex volume maximisation.  Runs on a SIVM
// context (pmf_set_option "sivm_gsat"); the host loop is pmf_host_gsat.h.
//
// The reference tests one sample at a time: with D the l2 distances among the k current vertices W and d the distances of the
// sample to them (l2 or l1: the constructor's measure), v[i] is the Cayley-Menger volume of "W without vertex i, plus the
// sample" (vol.py:24-34), and the sample replaces the first vertex of largest v[i] when that is >= V, the current volume.
// A rejected probe changes nothing, so a batch of probes is evaluated against the same simplex in one launch, the first
// accepted one is applied, and the probes behind it are evaluated again: the reference's sequence, decision for decision.
//
// Everything is float64 from the float32 values of the data: every decision compares two volumes.  The table holds distances,
// not squares, and a Cayley-Menger entry is the distance times itself, as in the reference (pdist, then d**2 in cmdet).
//
// k_gsat_probe   one workgroup per probe (at most PMF_GSAT_BATCH a launch).  A probe whose index is in `select` is marked
//   skipped (-2).  The candidate -- a strided column of the resident V, or the uploaded vector -- is staged PMF_GSAT_CHUNK
//   rows at a time, wave w sums the distances to the vertices w, w + 4, ... (gsat_distances).  Then each wave takes the
//   leave-one-out matrices i = w, w + 4, ...: (k + 1) x (k + 1) float64 in the wave's own LDS area (at 64 bases four areas of
//   33 800 bytes; the staging chunk lies over them, it is dead by then), LU with row pivoting (the matrices are indefinite),
//   |det| from the pivots folded factor by factor with f1 = 1 / (2^j (j!)^2), j = k - 1, so that neither over- nor underflows
//   on its own.  The determinants are formed directly: det(minor_i) = det(M) inv(M)_ii fails when the k + 1 points are
//   affinely dependent (rows < num_bases), and the reference has no such restriction.  A zero pivot column gives volume 0.
//   Result per probe: the first i of maximal v[i] if that is >= V, else -1; the volume; the k distances.
// k_gsat_commit  one workgroup behind it: the first probe of the launch with a slot >= 0 -- its column into W (the k x m image
//   of this path and the context's W), `select`, V, the log of accepted volumes, row and column of the distance table --, the
//   distances of the last probe evaluated up to it (the reference's D[k, :]), and the position for the host (count: none).
// k_gsat_take_w, k_gsat_table, k_gsat_volume  the start: the k x m image of the context's W, the table, V = cmdet(D).
#pragma once
#include "pmf_dev.h"

constexpr int PMF_GSAT_MAX_K = 64;
constexpr int PMF_GSAT_BATCH = 256;      // probes of a launch: one workgroup each, one per CU at 64 bases
constexpr int PMF_GSAT_CHUNK = 4096;     // rows of the candidate staged at a time (16 KiB)

struct GsatArgs {
  const float* V;          // the resident data [mp][np]
  int64_t np;
  int m, k, KP;
  const float* vec;        // non-null: the one candidate is this vector [m], not a data column
  float* Wg;               // [k][m] the vertices, one per row
  float* W;                // the context's W [mp][KP]
  double* Dt;              // [64][64] l2 distances among the vertices
  double* last;            // [64] distances of the last probe evaluated
  int* select;             // [k]
  double* Vcur;            // [0] the current volume
  const int64_t* idx;      // [count] the probes of this launch
  int* slots;              // [count] -2 skipped, -1 rejected, >= 0 the vertex replaced
  double* pvol;            // [PMF_GSAT_BATCH] the best volume of each probe
  double* pdist;           // [PMF_GSAT_BATCH][64] its distances
  double* log;             // the accepted volumes of the call
  int* ctl;                // [0] the position of the accepted probe in this launch, [1] entries of log
  int count;
  int l1;                  // the measure of the bordered distances: 0 l2, 1 l1
};

// one wave: its LDS stores before, other lanes' loads behind
__device__ __forceinline__ void gsat_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// out[j] = distance of x (m values, `stride` apart) to vertex j, j < k, float64 from the float32 values; the whole workgroup
// (256 threads); xs: PMF_GSAT_CHUNK floats of LDS.  The order of every sum is fixed: the same bits whoever calls.
__device__ __forceinline__ void gsat_distances(const float* __restrict__ x, const int64_t stride, const float* __restrict__ Wg, const int m,
                                               const int k, const bool l1, float* xs, double* out) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < PMF_GSAT_MAX_K) out[tid] = 0.0;
  for (int r0 = 0; r0 < m; r0 += PMF_GSAT_CHUNK) {
    const int len = min(PMF_GSAT_CHUNK, m - r0);
    __syncthreads();                             // the chunk before is consumed
    for (int r = tid; r < len; r += 256) xs[r] = x[(int64_t)(r0 + r) * stride];
    __syncthreads();
    for (int j = wv; j < k; j += 4) {
      const float* w = Wg + (int64_t)j * m + r0;
      double s = 0.0;
      for (int r = lane; r < len; r += 64) {
        const double d = (double)w[r] - (double)xs[r];
        s += l1 ? fabs(d) : d * d;
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) out[j] += s;                // (this wave alone touches out[j])
    }
  }
  __syncthreads();
  if (tid < k && !l1) out[tid] = sqrt(out[tid]);
  __syncthreads();
}

// One wave: the Cayley-Menger volume sqrt(|f1 det|) of k points -- the vertices without `skip`, then the candidate (point k,
// distances cd); skip = k: the k vertices themselves.  A: (k + 1) rows of LD doubles in LDS.
__device__ __forceinline__ double gsat_cm_volume(double* A, const int LD, const int k, const int skip, const double* __restrict__ Dt,
                                                 const double* cd, const int lane) {
  const int T = k + 1;
  for (int a = 0; a < T; ++a) {
    const int p = a - 1 + (a - 1 >= skip ? 1 : 0);
    for (int b = lane; b < T; b += 64) {
      const int q = b - 1 + (b - 1 >= skip ? 1 : 0);
      double v;
      if (a == b) v = 0.0;
      else if (a == 0 || b == 0) v = 1.0;
      else {
        const double d = p == k ? cd[q] : q == k ? cd[p] : Dt[p * PMF_GSAT_MAX_K + q];
        v = d * d;
      }
      A[a * LD + b] = v;
    }
  }
  gsat_wave_sync();
  double scale = 1.0;                            // |piv_0| |piv_k| prod_{p = 1 .. k - 1} |piv_p| / (2 p^2) = |f1 det|
  for (int p = 0; p < T; ++p) {
    // the pivot: the largest modulus in column p from row p down, the lowest row on a tie
    double best = -1.0;
    int br = p;
    for (int r = p + lane; r < T; r += 64) {
      const double v = fabs(A[r * LD + p]);
      if (v > best) { best = v; br = r; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double ov = __shfl_xor(best, o);
      const int orow = __shfl_xor(br, o);
      if (ov > best || (ov == best && orow < br)) { best = ov; br = orow; }
    }
    if (!(best > 0.0)) return 0.0;               // (the same in every lane) a zero column: the points are affinely dependent
    if (br != p) {
      for (int j = lane; j < T; j += 64) {
        const double u = A[p * LD + j];
        A[p * LD + j] = A[br * LD + j];
        A[br * LD + j] = u;
      }
      gsat_wave_sync();
    }
    const double piv = A[p * LD + p];
    scale *= (p >= 1 && p <= k - 1) ? fabs(piv) / (2.0 * (double)p * (double)p) : fabs(piv);
    for (int r = p + 1 + lane; r < T; r += 64) A[r * LD + p] /= piv;
    gsat_wave_sync();
    for (int j = p + 1 + lane; j < T; j += 64) {
      const double pj = A[p * LD + j];
      for (int r = p + 1; r < T; ++r) A[r * LD + j] = fma(-A[r * LD + p], pj, A[r * LD + j]);
    }
    gsat_wave_sync();
  }
  return sqrt(scale);
}

// dynamic LDS of k_gsat_probe: four wave areas, and at least the staging chunk
static inline size_t gsat_probe_smem(int k) {
  const size_t areas = (size_t)4 * (k + 1) * ((k + 1) | 1) * sizeof(double);
  const size_t chunk = (size_t)PMF_GSAT_CHUNK * sizeof(float);
  return areas > chunk ? areas : chunk;
}

__global__ __launch_bounds__(256) void k_gsat_probe(const GsatArgs a) {
  extern __shared__ __attribute__((aligned(16))) double gsat_lds[];
  __shared__ double cd[PMF_GSAT_MAX_K], vols[PMF_GSAT_MAX_K];
  __shared__ int s_skip;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x;
  const int k = a.k;
  const int64_t idx = a.vec ? -1 : a.idx[b];
  if (tid == 0) s_skip = 0;
  __syncthreads();
  if (!a.vec && tid < k && (int64_t)a.select[tid] == idx) s_skip = 1;
  __syncthreads();
  if (s_skip) {                                  // (the whole workgroup)
    if (tid == 0) { a.slots[b] = -2; a.pvol[b] = 0.0; }
    return;
  }
  gsat_distances(a.vec ? a.vec : a.V + idx, a.vec ? 1 : a.np, a.Wg, a.m, k, a.l1 != 0, reinterpret_cast<float*>(gsat_lds), cd);

  const int LD = (k + 1) | 1;
  double* A = gsat_lds + (size_t)wv * (k + 1) * LD;
  for (int i = wv; i < k; i += 4) {
    const double v = gsat_cm_volume(A, LD, k, i, a.Dt, cd, lane);
    if (lane == 0) vols[i] = v;
  }
  __syncthreads();
  if (tid < 64) {                                // np.argmax: the first of the largest
    double v = tid < k ? vols[tid] : -1.0;
    int r = tid;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double ov = __shfl_xor(v, o);
      const int orow = __shfl_xor(r, o);
      if (ov > v || (ov == v && orow < r)) { v = ov; r = orow; }
    }
    if (tid == 0) {
      a.slots[b] = v >= a.Vcur[0] ? r : -1;      // a tie with V swaps (sivm_gsat.py:102-105)
      a.pvol[b] = v;
    }
  }
  if (tid < k) a.pdist[b * PMF_GSAT_MAX_K + tid] = cd[tid];
}

__global__ __launch_bounds__(256) void k_gsat_commit(const GsatArgs a) {
  __shared__ float xs[PMF_GSAT_CHUNK];
  __shared__ double cd[PMF_GSAT_MAX_K];
  __shared__ int s_pos, s_last;
  const int tid = threadIdx.x;
  const int k = a.k, m = a.m;
  if (tid == 0) { s_pos = a.count; s_last = -1; }
  __syncthreads();
  if (tid < a.count && a.slots[tid] >= 0) atomicMin(&s_pos, tid);
  __syncthreads();
  const int pos = s_pos;
  if (tid < a.count && tid <= pos && a.slots[tid] != -2) atomicMax(&s_last, tid);
  __syncthreads();
  const int lastp = s_last;
  if (lastp >= 0 && tid < k) a.last[tid] = a.pdist[lastp * PMF_GSAT_MAX_K + tid];
  if (tid == 0) a.ctl[0] = pos;
  if (pos >= a.count) return;                    // (the whole workgroup) every probe of the launch is rejected or skipped

  const int s = a.slots[pos];
  const float* x = a.vec ? a.vec : a.V + a.idx[pos];
  const int64_t stride = a.vec ? 1 : a.np;
  float* ws = a.Wg + (int64_t)s * m;
  for (int r = tid; r < m; r += 256) {
    const float v = x[(int64_t)r * stride];
    ws[r] = v;
    a.W[(int64_t)r * a.KP + s] = v;
  }
  if (tid == 0) {
    if (!a.vec) a.select[s] = (int)a.idx[pos];   // (online_update_w leaves `select` alone: sivm_gsat.py:105-115)
    a.Vcur[0] = a.pvol[pos];
    const int n = a.ctl[1];
    a.log[n] = a.pvol[pos];
    a.ctl[1] = n + 1;
  }
  __syncthreads();                               // the new vertex is in place for the whole workgroup
  gsat_distances(ws, 1, a.Wg, m, k, false, xs, cd);   // pdist stays l2 (sivm_gsat.py:107)
  if (tid < k) {
    const double d = tid == s ? 0.0 : cd[tid];
    a.Dt[s * PMF_GSAT_MAX_K + tid] = d;
    a.Dt[tid * PMF_GSAT_MAX_K + s] = d;
  }
}

// ---- the start: vertex s of the context's W as row s of the image (one workgroup per vertex), the table's row s, V ----------
__global__ __launch_bounds__(256) void k_gsat_take_w(const GsatArgs a) {
  const int s = blockIdx.x;
  for (int r = threadIdx.x; r < a.m; r += 256) a.Wg[(int64_t)s * a.m + r] = a.W[(int64_t)r * a.KP + s];
}

__global__ __launch_bounds__(256) void k_gsat_table(const GsatArgs a) {
  __shared__ float xs[PMF_GSAT_CHUNK];
  __shared__ double cd[PMF_GSAT_MAX_K];
  const int s = blockIdx.x, tid = threadIdx.x;
  gsat_distances(a.Wg + (int64_t)s * a.m, 1, a.Wg, a.m, a.k, false, xs, cd);
  if (tid < a.k) a.Dt[s * PMF_GSAT_MAX_K + tid] = tid == s ? 0.0 : cd[tid];
}

__global__ __launch_bounds__(64) void k_gsat_volume(const GsatArgs a) {
  constexpr int LDMAX = (PMF_GSAT_MAX_K + 1) | 1;
  __shared__ double A[(PMF_GSAT_MAX_K + 1) * LDMAX];
  const double v = gsat_cm_volume(A, (a.k + 1) | 1, a.k, a.k, a.Dt, a.last, threadIdx.x);   // (no candidate: a.last is never read)
  if (threadIdx.x == 0) a.Vcur[0] = v;
}
