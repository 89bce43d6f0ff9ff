// pmf_host_products.h -- launchers of the row / column products (k_rowgemm*, k_colgemm*; the chunked forms over more than PMF_WIDE_K columns), the float64 H and G = H H^T
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// ---- kernel launch helpers --------------------------------------------------------------
// Grid of the element-wise kernels (256 threads, grid-stride loops): one thread per element up to 2^30 threads -- a launch of
// more than 2^32 threads wraps without an error (found with a 36 Mi x 256 matrix, tests/sweeps/huge_probe.py).
static inline unsigned elem_grid(int64_t count) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((count + 255) / 256, (int64_t)1 << 22));
}

template <int NT, int EPI>
int launch_rowgemm(pmf_ctx* c, const float* A, int64_t lda, int kdimA, const float* B, int64_t ldb,
                   float* W, const float* G, float* C, int64_t rows_p = -1, int64_t mvalid = -1, int64_t ldc = 0) {
  if (rows_p < 0) { rows_p = c->mp; mvalid = c->m; }
  if (ldc == 0) ldc = 16 * NT;
  const float lamb = (float)c->lamb_w;
  if constexpr (EPI == EPI_STORE || EPI == EPI_NMF_W || EPI == EPI_BNMF_W || EPI == EPI_RNMF_W) {
    if (c->opt_rowgemm_stream && kdimA % 128 == 0) {
      // long contraction: A straight into registers, requests interleaved with the MFMAs (pmf_tiled.h)
      constexpr int RB = NT <= 4 ? 4 : 2;
      const int ntiles = (int)(rows_p / (16 * RB));
      // persistent workgroups, two per CU of a 256-CU part (a fixed count; at 128 bases with the Den product one group each)
      const int ngroups = (ntiles + 3) / 4;
      const bool single = (EPI != EPI_STORE) && NT > 4;
      const unsigned grid = (unsigned)(single ? ngroups : std::min(ngroups, 512));
      const size_t ssm = rowgemm_stream_smem_bytes<NT, EPI, false>();
      if (ssm > 64 * 1024) {
        static bool sattr_dev[PMF_MAX_DEVICES] = {};
        bool& sattr = sattr_dev[pmf_current_device()];
        if (!sattr) {
          HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rowgemm_stream<NT, RB, EPI>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)ssm));
          sattr = true;
        }
      }
      hipLaunchKernelGGL((k_rowgemm_stream<NT, RB, EPI>), dim3(grid), dim3(256), ssm, c->stream, A, lda, kdimA, B, ldb, W, G, C, ldc, lamb, mvalid,
                         c->k, ntiles, (int64_t)(16 * NT));
      HIPCHK(c, hipGetLastError());
      return PMF_OK;
    }
  }
  const size_t smem = rowgemm_smem_bytes<NT>();
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rowgemm<NT, EPI>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    attr_done = true;
  }
  const int ntiles = (int)(rows_p / 64);
  const int tpw = ntiles >= 8192 ? 8 : ntiles >= 2048 ? 4 : ntiles >= 1024 ? 2 : 1;   // consecutive tiles per workgroup
  hipLaunchKernelGGL((k_rowgemm<NT, EPI>), dim3((unsigned)((ntiles + tpw - 1) / tpw)), dim3(256), smem, c->stream,
                     A, lda, kdimA, B, ldb, W, G, C, ldc, lamb, mvalid, c->k, ntiles, tpw);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

template <int EPI>
int rowgemm_one(pmf_ctx* c, const float* A, int64_t lda, int kdimA, const float* B, int64_t ldb,
                float* W, const float* G, float* C, int64_t rows_p = -1, int64_t mvalid = -1) {
  if (c->nb > 1) {            // num_bases > 128: the plain product in blocks of 128 bases, C is [.][KP]
    if (EPI != EPI_STORE) return fail(c, PMF_EINVAL, "rowgemm: only the plain product runs in base blocks");
    for (int b = 0; b < c->nb; ++b)
      PMFCHK((launch_rowgemm<8, EPI_STORE>(c, A, lda, kdimA, B + (size_t)b * 128 * ldb, ldb, nullptr, nullptr, C + b * 128,
                                           rows_p, mvalid, c->KP)));
    return PMF_OK;
  }
  switch (c->NT) {
    case 1: return launch_rowgemm<1, EPI>(c, A, lda, kdimA, B, ldb, W, G, C, rows_p, mvalid);
    case 2: return launch_rowgemm<2, EPI>(c, A, lda, kdimA, B, ldb, W, G, C, rows_p, mvalid);
    case 4: return launch_rowgemm<4, EPI>(c, A, lda, kdimA, B, ldb, W, G, C, rows_p, mvalid);
    case 8: return launch_rowgemm<8, EPI>(c, A, lda, kdimA, B, ldb, W, G, C, rows_p, mvalid);
  }
  return fail(c, PMF_EINVAL, "bad NT");
}

// A product over the columns of V is ONE accumulation chain of kdim / 4 MFMA steps per output element, and the fp32 MFMA
// does not round its running sum to nearest: the chain loses a fraction of about 1.5e-16 * steps^2 of the sum (measured on
// uniform data, tests/sweeps/wide_scan.py: V H^T biased by -2e-7 at 32 768 columns, -3.2e-6 at 131 072, -4.2e-5 at 524 288,
// -1.5e-4 at 10^6 -- W comes out scaled by that factor and H by its inverse, the fit itself is unaffected).  Products over
// more than PMF_WIDE_K columns are therefore formed in chunks of PMF_WIDE_K columns whose results are added in float32
// (round to nearest): the bias stays at the 65 536-column level (1e-6) whatever n.  Shapes up to 65 536 columns run as before.
constexpr int PMF_WIDE_K = 65536;

template <int EPI>
int rowgemm(pmf_ctx* c, const float* A, int64_t lda, int kdimA, const float* B, int64_t ldb,
            float* W, const float* G, float* C, int64_t rows_p = -1, int64_t mvalid = -1) {
  if constexpr (EPI == EPI_STORE) {
    if (kdimA > PMF_WIDE_K) {
      const int64_t rp = rows_p < 0 ? c->mp : rows_p;
      const int64_t count = rp * c->KP;
      PMFCHK(dgrow(c, &c->dWideT, &c->wide_cap, count));
      for (int k0 = 0; k0 < kdimA; k0 += PMF_WIDE_K) {
        const int kc = std::min(PMF_WIDE_K, kdimA - k0);
        PMFCHK(rowgemm_one<EPI_STORE>(c, A + k0, lda, kc, B + k0, ldb, W, G, k0 == 0 ? C : c->dWideT, rows_p, mvalid));
        if (k0 > 0) {
          hipLaunchKernelGGL(k_acc_f32, dim3(elem_grid(count / 4)), dim3(256), 0, c->stream, C, c->dWideT, count);
          HIPCHK(c, hipGetLastError());
        }
      }
      return PMF_OK;
    }
  }
  return rowgemm_one<EPI>(c, A, lda, kdimA, B, ldb, W, G, C, rows_p, mvalid);
}

// The W rules of NMF / BNMF / RNMF over more than PMF_WIDE_K columns: Num = X H^T in chunks (above), Den = W G by a small
// kernel, the rule element by element -- what the one-launch forms (update rule as the product's epilogue) cannot do in chunks.
int wide_update_w_rows(pmf_ctx* c, const float* X, float* Wr, int64_t rows_p, int64_t mvalid) {
  const int64_t count = rows_p * c->KP;
  if (c->wide_nd_cap < count) {
    c->wide_nd_cap = 0;
    PMFCHK(dgrow(c, &c->dWideN, (size_t)count));
    PMFCHK(dgrow(c, &c->dWideD, (size_t)count));
    c->wide_nd_cap = count;
  }
  float *Num = c->dWideN, *Den = c->dWideD;
  PMFCHK(rowgemm<EPI_STORE>(c, X, c->np, c->np, c->dH, c->np, nullptr, nullptr, Num, rows_p, mvalid));
  hipLaunchKernelGGL(k_den_small, dim3(elem_grid(count)), dim3(256), 0, c->stream, Wr, c->dG, Den, rows_p, c->KP);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_nmf_w_elem, dim3(elem_grid(count)), dim3(256), 0, c->stream, Wr, Num, Den, count,
                     c->algo == PMF_ALGO_BNMF ? 1 : c->algo == PMF_ALGO_RNMF ? 2 : 0, (float)c->lamb_w, c->KP, mvalid, c->k);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

// Partials of (W^T X | W^T W) over row chunks into c->dSlab: X [rows_p][xn] (ldx), W [rows_p][.] (ldw), chunks of rpc rows.
// k_colgemm_stream where it applies (NT = 4, or NT = 8 without S; rpc a multiple of its stage), else k_colgemm.
template <int NT, bool WITH_S>
int launch_colgemm(pmf_ctx* c, const float* X, int64_t ldx, int xn, const float* W, int64_t ldw, int64_t rows_p, int rpc, int nch,
                   float* slab = nullptr) {
  if (!slab) slab = c->dSlab;
  const dim3 grid((unsigned)nch, X ? (unsigned)((xn + 255) / 256) : 1u);
  constexpr int SR = NT == 4 ? 64 : 32;
  const bool stream_ok = c->opt_colgemm_stream && X != nullptr && rpc % SR == 0 && rows_p % SR == 0;
  const size_t smem = (size_t)2 * SR * (16 * NT + 4) * sizeof(float);
  if constexpr (NT == 4 || (NT == 8 && !WITH_S)) {
    if (stream_ok) {
      hipLaunchKernelGGL((k_colgemm_stream<NT, WITH_S>), grid, dim3(256), smem, c->stream, X, ldx, xn, W, ldw, rows_p, rpc, slab,
                         (int64_t)xn + 16 * NT, 0);
      HIPCHK(c, hipGetLastError());
      return PMF_OK;
    }
  }
  if constexpr (NT == 8 && WITH_S) {
    // 64 < num_bases <= 128: with the S tiles k_colgemm<8> holds 192 accumulator registers; the stream kernel forms P and,
    // as a second product with W in V's place, S -- into the same slabs (columns [xn, xn + 128))
    if (stream_ok) {
      hipLaunchKernelGGL((k_colgemm_stream<8, false>), grid, dim3(256), smem, c->stream, X, ldx, xn, W, ldw, rows_p, rpc, slab,
                         (int64_t)xn + 128, 0);
      hipLaunchKernelGGL((k_colgemm_stream<8, false>), dim3((unsigned)nch, 1u), dim3(256), smem, c->stream, W, ldw, 128, W, ldw, rows_p, rpc,
                         slab, (int64_t)xn + 128, xn);
      HIPCHK(c, hipGetLastError());
      return PMF_OK;
    }
  }
  hipLaunchKernelGGL((k_colgemm<NT, WITH_S>), grid, dim3(256), 0, c->stream, X, ldx, xn, W, ldw, rows_p, rpc, slab);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

int colgemm_rows(pmf_ctx* c, const float* X, const float* W, int64_t rows_p, int rpc, int nch) {
  switch (c->NT) {
    case 1: return launch_colgemm<1, true>(c, X, c->np, c->np, W, c->KP, rows_p, rpc, nch);
    case 2: return launch_colgemm<2, true>(c, X, c->np, c->np, W, c->KP, rows_p, rpc, nch);
    case 4: return launch_colgemm<4, true>(c, X, c->np, c->np, W, c->KP, rows_p, rpc, nch);
    case 8: return launch_colgemm<8, true>(c, X, c->np, c->np, W, c->KP, rows_p, rpc, nch);
  }
  return fail(c, PMF_EINVAL, "bad NT");
}

int colgemm(pmf_ctx* c, bool with_v = true) {
  const float* Vp = with_v ? (c->algo == PMF_ALGO_RNMF ? c->dD : c->dV) : nullptr;
  return colgemm_rows(c, Vp, c->dW, c->mp, c->rows_per_chunk, c->nchunks);
}

int64_t ps_elems(const pmf_ctx* c) { return (int64_t)c->KP * (c->np + c->KP); }

// SNMF keeps H in float64 on the device (num_bases <= 128)
static inline bool h_in_f64(const pmf_ctx* c) { return (c->algo == PMF_ALGO_SNMF || c->algo == PMF_ALGO_CNMF) && c->nb == 1; }

// dHd exists and agrees with dH: entries whose rounding is not the float32 H any more are replaced by the widened float32 value
int ensure_hd(pmf_ctx* c) {
  if (!c->dHd) {
    PMFCHK(dalloc(c, &c->dHd, (size_t)c->KP * c->np));
    PMFCHK(dalloc(c, &c->dSd, (size_t)c->KP * c->KP));
    c->hd_synced = false;
  }
  if (c->hd_synced) return PMF_OK;
  const int64_t E = (int64_t)c->KP * c->np;
  hipLaunchKernelGGL(k_hd_sync, dim3((unsigned)std::min<int64_t>((E + 255) / 256, 1024)), dim3(256), 0, c->stream, c->dH, c->dHd, E, c->hd_force ? 1 : 0);
  HIPCHK(c, hipGetLastError());
  c->hd_synced = true; c->hd_force = false;
  return PMF_OK;
}

int ensure_gram(pmf_ctx* c, double pad_diag) {
  if (c->g_valid && c->g_parts > 0) {            // k_nmf_h_gram left partial sums: add them up
    const int E = c->KP * c->KP;
    hipLaunchKernelGGL(k_sum_gparts, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, c->stream, c->dGpart, c->g_parts, E, c->dG);
    HIPCHK(c, hipGetLastError());
    c->g_parts = 0;
  }
  if (c->g_valid) return PMF_OK;
  c->g_parts = 0;   // (a count left behind by an H step whose H has been replaced since: the partials in dGpart are that H's)
  const bool h64 = h_in_f64(c);
  if (h64) PMFCHK(ensure_hd(c));                 // SNMF: G = Hd Hd^T, the float64 H
  dim3 grid((unsigned)(c->KP / 16), (unsigned)(c->KP / 16));
  const int ks = c->np >= 2048 && c->np % 512 == 0 ? 8 : c->np >= 512 && c->np % 256 == 0 ? 4 : 1;   // column slices (wide H)
  if (ks > 1 && c->nb == 1) {
    if (!c->dGramPart) {
      PMFCHK(dalloc(c, &c->dGramPart, (size_t)8 * c->KP * c->KP));
      PMFCHK(dalloc(c, &c->dGramTickets, (size_t)(c->KP / 16) * (c->KP / 16)));
    }
    grid.z = (unsigned)ks;
    if (h64) hipLaunchKernelGGL(k_gram_splitk<double>, grid, dim3(256), 0, c->stream, c->dHd, (int64_t)c->np, c->np, c->KP, c->k, pad_diag, c->dG, c->dGd,
                                c->dGramPart, c->dGramTickets);
    else hipLaunchKernelGGL(k_gram_splitk<float>, grid, dim3(256), 0, c->stream, c->dH, (int64_t)c->np, c->np, c->KP, c->k, pad_diag, c->dG, c->dGd,
                            c->dGramPart, c->dGramTickets);
  } else {
    if (h64) hipLaunchKernelGGL(k_gram<double>, grid, dim3(256), 0, c->stream, c->dHd, (int64_t)c->np, c->np, c->KP, c->k,
                                pad_diag, c->dG, c->dGd);
    else hipLaunchKernelGGL(k_gram<float>, grid, dim3(256), 0, c->stream, c->dH, (int64_t)c->np, c->np, c->KP, c->k,
                            pad_diag, c->dG, c->dGd);
  }
  HIPCHK(c, hipGetLastError());
  c->g_valid = true;
  return PMF_OK;
}

}  // namespace
