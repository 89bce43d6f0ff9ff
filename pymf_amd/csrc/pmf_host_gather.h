// pmf_host_gather.h -- pmf_set_v_gather_f32: the refusals, the staged index array, the launch of k_gather_cols (pmf_gather.h) between
// the two events that order the source's stream and the destination's; pmf_get_v_dense_f32's check.  What precedes and follows
// the fill of dV -- the halves every dense fill shares -- is dense_v_begin / dense_v_end in pmf_api.hip.
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// dense float32 data resident on c?  nullptr, or what is in the way ("who: <what>" is the caller's message)
const char* gather_no_dense(const pmf_ctx* c) {
  if (c->v_csr) return "holds CSR data; dense resident data only";
  if (c->v_csc) return "holds CSC data; dense resident data only";
  if (c->st_active) return "is in streamed mode (a pmf_stream_* pass is open); dense resident data only";
  if (!c->have_v || !c->dV) return "has no data (streamed data is never resident; pmf_set_v_dense_* first)";
  return nullptr;
}

// Every refusal of pmf_set_v_gather_f32, decided on the host: nothing of dst has been touched when one of them returns.  On
// success idx32 holds the indices as the kernel reads them (empty: the whole copy).
int gather_check(pmf_ctx* dst, pmf_ctx* src, const int64_t* idx, int64_t nsel, std::vector<int32_t>* idx32) {
  const std::string w("pmf_set_v_gather_f32: ");
  if (!src) return fail(dst, PMF_EINVAL, w + "src is NULL");
  if (src == dst) return fail(dst, PMF_EINVAL, w + "src and dst are the same context");
  if (src->device != dst->device) return fail(dst, PMF_EINVAL, w + "src and dst are on different devices");
  if (multi_rank(src) || src->nranks > 1) return fail(dst, PMF_EINVAL, w + "src belongs to a multi-rank world; one rank only");
  if (multi_rank(dst) || dst->nranks > 1) return fail(dst, PMF_EINVAL, w + "dst belongs to a multi-rank world; one rank only");
  if (const char* why = gather_no_dense(src)) return fail(dst, PMF_EINVAL, w + "src " + why);
  if (dst->st_active) return fail(dst, PMF_EINVAL, w + "dst is in streamed mode (a pmf_stream_* pass is open)");
  if (src->m != dst->m) return fail(dst, PMF_EINVAL, w + "src->m != dst->m (rows " + std::to_string(src->m) + " and " + std::to_string(dst->m) + ")");
  if (nsel != dst->n) return fail(dst, PMF_EINVAL, w + "nsel != dst->n (" + std::to_string(nsel) + " and " + std::to_string(dst->n) + ")");
  idx32->clear();
  if (!idx) {
    if (nsel != src->n) return fail(dst, PMF_EINVAL, w + "idx is NULL (the whole copy) and nsel != src->n (" + std::to_string(nsel) + " and " + std::to_string(src->n) + ")");
    return PMF_OK;
  }
  idx32->resize((size_t)nsel);
  for (int64_t j = 0; j < nsel; ++j) {
    if (idx[j] < 0 || idx[j] >= src->n)
      return fail(dst, PMF_EINVAL, w + "index out of range: idx[" + std::to_string(j) + "] = " + std::to_string(idx[j]) + ", src->n = " + std::to_string(src->n));
    (*idx32)[(size_t)j] = (int32_t)idx[j];
  }
  return PMF_OK;
}

// the index array on the device (dst's own buffer, kept between calls); returns with the copy done: idx32 may go
int gather_stage_idx(pmf_ctx* dst, const std::vector<int32_t>& idx32) {
  if (idx32.empty()) return PMF_OK;
  PMFCHK(dgrow(dst, &dst->dGaIdx, &dst->ga_idx_cap, (int64_t)idx32.size(), 1, /*sync=*/true));
  HIPCHK(dst, hipMemcpyAsync(dst->dGaIdx, idx32.data(), idx32.size() * sizeof(int32_t), hipMemcpyHostToDevice, dst->stream));
  HIPCHK(dst, hipStreamSynchronize(dst->stream));
  return PMF_OK;
}

void gather_stat(pmf_ctx* c, bool ident, int64_t nsel) {
  if (!c->profile || c->stat.site != SITE_GATHER) return;
  c->stat.name = ident ? "k_gather_cols<ident>" : "k_gather_cols<idx>";
  c->stat.flops = c->stat.exec_flops = 0.0;
  c->stat.bytes = 8.0 * (double)c->m * (double)nsel + (ident ? 0.0 : 4.0 * (double)nsel);   // every value read and written once, the indices read
}

// dst->dV <- the chosen columns of src->dV.  The two contexts have streams of their own: what src's stream holds completes
// before the kernel reads (event 0), and the kernel completes before anything enqueued on src's stream from now on runs
// (event 1) -- no host wait, nothing device-wide.
int gather_fill(pmf_ctx* dst, pmf_ctx* src, bool ident, int64_t nsel) {
  for (hipEvent_t& e : dst->ev_ga)
    if (!e) HIPCHK(dst, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  GatherArgs a{};
  a.src = reinterpret_cast<const uint32_t*>(src->dV); a.dst = reinterpret_cast<uint32_t*>(dst->dV); a.idx = dst->dGaIdx;
  a.snp = src->np; a.dnp = dst->np;
  a.m = (int)dst->m; a.mp = (int)dst->mp; a.n = (int)src->n; a.nsel = (int)nsel;
  const int64_t groups = a.dnp / 4;
  a.tx_log2 = groups >= 256 ? 8 : groups >= 64 ? 6 : 4;
  const int tx = 1 << a.tx_log2, ty = 256 >> a.tx_log2;
  const int64_t gx = (groups + tx - 1) / tx;
  const int64_t want_y = std::max<int64_t>(1, (2048 + gx - 1) / gx);      // some 8 workgroups per compute unit where the rows allow it
  a.rows_per_wg = (int)round_up((dst->mp + want_y - 1) / want_y, (int64_t)PMF_GATHER_ROWS_IN_FLIGHT * ty);
  const int64_t gy = (dst->mp + a.rows_per_wg - 1) / a.rows_per_wg;
  HIPCHK(dst, hipEventRecord(dst->ev_ga[0], src->stream));
  HIPCHK(dst, hipStreamWaitEvent(dst->stream, dst->ev_ga[0], 0));
  gather_stat(dst, ident, nsel);
  stat_begin(dst, SITE_GATHER);
  if (ident) hipLaunchKernelGGL(k_gather_cols<true>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, dst->stream, a);
  else hipLaunchKernelGGL(k_gather_cols<false>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, dst->stream, a);
  stat_end(dst, SITE_GATHER);
  HIPCHK(dst, hipGetLastError());
  HIPCHK(dst, hipEventRecord(dst->ev_ga[1], dst->stream));
  HIPCHK(dst, hipStreamWaitEvent(src->stream, dst->ev_ga[1], 0));
  return PMF_OK;
}

}  // namespace
