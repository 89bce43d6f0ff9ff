// pmf_host_nmf_csr.h -- NMF on CSR data: the upload with its transposed copy, the two half steps on k_nmf_sp_step (kernel: pmf_nmf_csr.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
//
// State (pmf_ctx): the CSR arrays of V (dIndptr ...) and of V^T (dTIndptr ...); W in dW; H as H^T [np][KP] in dHT -- the working
// copy of the H steps, dH follows it before the API call that ran them returns (nmf_csr_sync_h), so pmf_get_h / pmf_set_h and
// every other reader of dH keep their meaning; G = H H^T in dG (g_valid) and S = W^T W in dSw (sw_valid).  A half step leaves
// the Gram matrix of the factor it wrote, which is the G of the next half step: an iteration is two launches of the kernel
// and two slab sums.  Only the first half step of a call (or one behind a factor from outside) takes its G from a Gram pass
// over the resident factor.  No dense V, no (P | S): ps_valid stays off.
#pragma once

namespace {

// dense data came back to the context: the name of its dense path again; the CSR side arrays stay until the next upload
void nmf_csr_left(pmf_ctx* c) {
  if (c->path_dense.empty()) return;
  c->path = c->path_dense;
  c->path_dense.clear();
  choose_stat_site(c, false);
}

// The CSR image of an m x n matrix as pmf_set_v_csr_f32 takes it, checked on the host before anything is uploaded: the kernels
// use a column index as an LDS index and the differences of indptr as trip counts.  Entries of a row may come in any order and
// repeat (they add up).  nullptr: well-formed; else what is wrong.
const char* csr_check(int64_t m, int64_t n, const int64_t* indptr, const int32_t* indices, int64_t nnz) {
  if (indptr[0] != 0 || indptr[m] != nnz) return "indptr[0] must be 0 and indptr[m] must be nnz";
  for (int64_t r = 0; r < m; ++r)
    if (indptr[r + 1] < indptr[r]) return "indptr must not decrease";
  for (int64_t e = 0; e < nnz; ++e)
    if (indices[e] < 0 || indices[e] >= n) return "column index out of range";
  return nullptr;
}

// The CSR arrays of V^T from those of V (checked by csr_check): a stable counting sort of the entries by column, on the host --
// rows ascending within a column, entries of one (row, column) pair in stored order (a fixed summation order).  tip [np + 1]
// (columns >= n: empty rows of V^T), tind and tval [nnz]; ip [mp + 1] = indptr with the pad rows empty.
struct CsrPair {
  std::vector<int64_t> ip, tip;
  std::vector<int32_t> tind;
  std::vector<float> tval;
};
void csr_transpose_host(const pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz, CsrPair& p);
int csr_upload_pair(pmf_ctx* c, const CsrPair& p, const int32_t* indices, const float* vals, int64_t nnz);   // (both below nmf_csr_set_v)

// pmf_set_v_csr_f32 on an NMF context.  The H step needs the rows of V^T: csr_transpose_host, uploaded next to the CSR arrays.
int nmf_csr_set_v(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz) {
  if (c->nb > 1) return fail(c, PMF_EINVAL, "NMF on CSR data: num_bases > 128 is not supported by this build");
  if (c->nranks > 1 || multi_rank(c)) return fail(c, PMF_EINVAL, "NMF on CSR data: one rank only in this build (nranks > 1)");
  if (const char* why = csr_check(c->m, c->n, indptr, indices, nnz)) return fail(c, PMF_EINVAL, std::string("pmf_set_v_csr_f32: ") + why);
  CsrPair p;
  csr_transpose_host(c, indptr, indices, vals, nnz, p);

  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->dHT) {
    int dev = 0, cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    // workgroups that fit a CU (LDS: the G image and the waves' tiles; at most 2048 threads), over the blocks of the longer side
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2048 / (64 * nmfsp_waves(c->NT)), (160 * 1024) / (int64_t)nmfsp_smem_bytes(c->NT)));
    const int64_t nblk = std::max<int64_t>(c->mp, c->np) / 16;
    c->sp_wgs_cap = (int)std::max<int64_t>(1, std::min<int64_t>((nblk + nmfsp_waves(c->NT) - 1) / nmfsp_waves(c->NT), cus * per_cu));
    PMFCHK(dalloc(c, &c->dHT, (size_t)c->np * c->KP));
    PMFCHK(dalloc(c, &c->dSw, (size_t)c->KP * c->KP));
    PMFCHK(dalloc(c, &c->dSpSlab, (size_t)c->sp_wgs_cap * c->KP * c->KP));
  }
  PMFCHK(csr_upload_pair(c, p, indices, vals, nnz));
  c->nnz = nnz; c->have_v = true; c->v_csr = true; c->csr_dense = false;
  v_replaced(c);
  // the dense paths that may have run since the last CSR upload keep dH and g_valid, not H^T and W^T W
  c->ht_valid = c->ht_newer = c->sw_valid = false;
  if (c->path_dense.empty()) c->path_dense = c->path;
  c->path = "nmf_csr_gather<" + std::to_string(c->NT) + ">";
  choose_stat_site(c, false);
  return PMF_OK;
}

void csr_transpose_host(const pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t nnz, CsrPair& p) {
  p.tip.assign((size_t)c->np + 1, 0);
  for (int64_t e = 0; e < nnz; ++e) ++p.tip[(size_t)indices[e] + 1];
  for (int64_t q = 0; q < c->np; ++q) p.tip[(size_t)q + 1] += p.tip[(size_t)q];
  p.tind.resize((size_t)nnz);
  p.tval.resize((size_t)nnz);
  {
    std::vector<int64_t> at(p.tip.begin(), p.tip.end() - 1);
    for (int64_t r = 0; r < c->m; ++r)
      for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
        const int64_t d = at[(size_t)indices[e]]++;
        p.tind[(size_t)d] = (int32_t)r;
        p.tval[(size_t)d] = vals[e];
      }
  }
  p.ip.resize((size_t)c->mp + 1);
  for (int64_t r = 0; r <= c->mp; ++r) p.ip[(size_t)r] = indptr[std::min(r, c->m)];
}

// both images onto the device (dIndptr ..., dTIndptr ...), the buffers sized anew; returns with the copies done
int csr_upload_pair(pmf_ctx* c, const CsrPair& p, const int32_t* indices, const float* vals, int64_t nnz) {
  PMFCHK(dgrow(c, &c->dIndptr, (size_t)c->mp + 1));
  PMFCHK(dgrow(c, &c->dIndices, (size_t)nnz));
  PMFCHK(dgrow(c, &c->dVals, (size_t)nnz));
  PMFCHK(dgrow(c, &c->dTIndptr, (size_t)c->np + 1));
  PMFCHK(dgrow(c, &c->dTIndices, (size_t)nnz));
  PMFCHK(dgrow(c, &c->dTVals, (size_t)nnz));
  HIPCHK(c, hipMemcpyAsync(c->dIndptr, p.ip.data(), p.ip.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->dTIndptr, p.tip.data(), p.tip.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  if (nnz) {
    HIPCHK(c, hipMemcpyAsync(c->dIndices, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dVals, vals, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dTIndices, p.tind.data(), (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dTVals, p.tval.data(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));       // (the host arrays may leave scope)
  return PMF_OK;
}

int nmf_csr_transpose(pmf_ctx* c, const float* A, int64_t lda, int rows, int cols, float* B, int64_t ldb) {
  hipLaunchKernelGGL(k_transpose_f32, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, c->stream, A, lda,
                     rows, cols, B, ldb);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

int nmf_csr_ensure_ht(pmf_ctx* c) {         // dHT = dH^T
  if (c->ht_valid) return PMF_OK;
  PMFCHK(nmf_csr_transpose(c, c->dH, c->np, c->KP, c->np, c->dHT, c->KP));
  c->ht_valid = true; c->ht_newer = false;
  return PMF_OK;
}

int nmf_csr_sync_h(pmf_ctx* c) {            // dH = dHT^T behind the H steps of a call
  if (!c->ht_newer) return PMF_OK;
  PMFCHK(nmf_csr_transpose(c, c->dHT, c->KP, c->np, c->KP, c->dH, c->np));
  c->ht_newer = false;
  return PMF_OK;
}

// S = W^T W of the resident W by the dense partial-sum kernel (the S part of its (P | S) slabs), summed into dSw
int nmf_csr_ensure_sw(pmf_ctx* c) {
  if (c->sw_valid) return PMF_OK;
  c->ps_valid = false;                      // (the slabs' P part is not formed)
  PMFCHK(colgemm(c, /*with_v=*/false));
  const int64_t cnt4 = (int64_t)c->KP * c->KP / 4;
  hipLaunchKernelGGL((k_reduce_slabs_block<float>), dim3((unsigned)((cnt4 + 63) / 64)), dim3(1024), 0, c->stream, c->dSlab + c->np,
                     c->nchunks, c->KP, c->np + c->KP, c->KP, c->dSw, (int64_t)c->KP, 0);
  HIPCHK(c, hipGetLastError());
  c->sw_valid = true;
  return PMF_OK;
}

// one half step: X (rows_p x KP) updated in place from the CSR rows, Y and G; the Gram matrix of the new X into `gram_out`
template <int NT>
int launch_nmf_sp_step(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t rows_p, const float* Y,
                       const float* G, float* X, float* gram_out) {
  constexpr int WAVES = nmfsp_waves(NT);
  const size_t smem = nmfsp_smem_bytes(NT);
  static bool attr_done_dev[PMF_MAX_DEVICES] = {};   // the attribute is per device
  bool& attr_done = attr_done_dev[pmf_current_device()];
  if (!attr_done) {
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nmf_sp_step<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    attr_done = true;
  }
  const int nblk = (int)(rows_p / 16);
  const int wgs = (int)std::max<int64_t>(1, std::min<int64_t>((nblk + WAVES - 1) / WAVES, c->sp_wgs_cap));
  const int nw = wgs * WAVES;
  stat_begin(c, SITE_CSR_PASS);
  hipLaunchKernelGGL((k_nmf_sp_step<NT>), dim3((unsigned)wgs), dim3(64 * WAVES), smem, c->stream, indptr, indices, vals, nblk / nw,
                     nblk % nw, Y, G, X, c->dSpSlab);
  stat_end(c, SITE_CSR_PASS);
  HIPCHK(c, hipGetLastError());
  const int64_t E = (int64_t)c->KP * c->KP;
  hipLaunchKernelGGL(k_reduce_slabs, dim3((unsigned)((E / 4 + 63) / 64)), dim3(1024), 0, c->stream, c->dSpSlab, wgs, E, gram_out,
                     (double*)nullptr, 0, 0, 0);
  HIPCHK(c, hipGetLastError());
  return PMF_OK;
}

int nmf_sp_step(pmf_ctx* c, const int64_t* indptr, const int32_t* indices, const float* vals, int64_t rows_p, const float* Y,
                const float* G, float* X, float* gram_out) {
  switch (c->NT) {
    case 1: return launch_nmf_sp_step<1>(c, indptr, indices, vals, rows_p, Y, G, X, gram_out);
    case 2: return launch_nmf_sp_step<2>(c, indptr, indices, vals, rows_p, Y, G, X, gram_out);
    case 4: return launch_nmf_sp_step<4>(c, indptr, indices, vals, rows_p, Y, G, X, gram_out);
    case 8: return launch_nmf_sp_step<8>(c, indptr, indices, vals, rows_p, Y, G, X, gram_out);
  }
  return fail(c, PMF_EINVAL, "bad NT");
}

// nmf.py:128-132 on the rows of V: X = W, Y = H^T, G = H H^T; leaves S = W^T W
int nmf_csr_update_w(pmf_ctx* c) {
  if (c->nb > 1 || !c->dHT) return fail(c, PMF_EINVAL, "NMF on CSR data: no device state (pmf_set_v_csr_f32)");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "NMF on CSR data: one rank only in this build");
  if (!c->g_valid) PMFCHK(nmf_csr_sync_h(c));
  PMFCHK(ensure_gram(c, 0.0));
  PMFCHK(nmf_csr_ensure_ht(c));
  c->sw_valid = false;
  PMFCHK(nmf_sp_step(c, c->dIndptr, c->dIndices, c->dVals, c->mp, c->dHT, c->dG, c->dW, c->dSw));
  c->sw_valid = true;
  c->num_valid = false;
  return PMF_OK;
}

// nmf.py:122-126 on the rows of V^T: X = H^T, Y = W, G = W^T W; leaves G = H H^T
int nmf_csr_update_h(pmf_ctx* c) {
  if (c->nb > 1 || !c->dHT) return fail(c, PMF_EINVAL, "NMF on CSR data: no device state (pmf_set_v_csr_f32)");
  if (multi_rank(c)) return fail(c, PMF_EINVAL, "NMF on CSR data: one rank only in this build");
  PMFCHK(nmf_csr_ensure_sw(c));
  PMFCHK(nmf_csr_ensure_ht(c));
  c->g_valid = false; c->g_parts = 0;
  PMFCHK(nmf_sp_step(c, c->dTIndptr, c->dTIndices, c->dTVals, c->np, c->dW, c->dSw, c->dHT, c->dG));
  c->ht_newer = true;                       // dH follows before the call returns (run_step, NmfLoopSteps::close, pmf_get_h_*)
  c->g_valid = true;
  c->num_valid = false; c->trace_ready = false; c->ps_valid = false;
  return PMF_OK;
}

}  // namespace
