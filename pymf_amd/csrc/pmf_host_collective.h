// pmf_host_collective.h -- slab sums, the cross-rank sums (one-shot IPC exchange, RCCL, host transport) and the per-iteration collective
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

int reduce_slabs(pmf_ctx* c, int nslabs) {
  const int64_t E = ps_elems(c);      // multiple of 4 (KP and np are multiples of 16)
  // NMFALS on one rank: the column QPs' Hessian S = W^T W leaves the same launch in float64 (with more ranks it has to come
  // from the ALL-REDUCED sums: k_hessian_from_ps behind the collective)
  const bool hess = c->want_hess && !multi_rank(c);
  hipLaunchKernelGGL(k_reduce_slabs, dim3((unsigned)((E / 4 + 63) / 64)), dim3(1024), 0, c->stream,
                     c->dSlab, nslabs, E, c->dPS, hess ? c->dGd : (double*)nullptr, c->np, c->KP, c->k);
  HIPCHK(c, hipGetLastError());
  if (hess) c->gd_is_s = true;
  return PMF_OK;
}

// Sum `count` floats (or doubles) at device pointer `p` over all ranks, in place, in stream order.
// Transport: the context's RCCL communicator (one ncclAllReduce on the library's stream); or, when the
// caller installed a host transport (pmf_set_host_allreduce: plumbing checks where the ranks cannot form
// an RCCL communicator, e.g. several ranks sharing one GPU), a blocking round trip through the host.
int allreduce_sum(pmf_ctx* c, void* p, size_t count, bool f64) {
  const size_t nbytes = count * (f64 ? sizeof(double) : sizeof(float));
  if (c->ipc.nranks > 1 && nbytes <= PMF_IPC_MAX_BYTES && count > 0) {
    // one kernel: every rank writes its partial into every peer's receive area and adds the N partials in rank order
    const unsigned seq = ++c->ipc_seq;
    const int64_t vec = (int64_t)(count + 1023) / 1024;                         // ~1024 elements per workgroup
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(vec, PMF_IPC_AR_MAX_WGS));
    if (f64) hipLaunchKernelGGL((k_ipc_allreduce<double>), dim3(grid), dim3(256), 0, c->stream, (double*)p, (int64_t)count, c->ipc, seq, c->dIpcErr, c->ipc_wait_ticks);
    else hipLaunchKernelGGL((k_ipc_allreduce<float>), dim3(grid), dim3(256), 0, c->stream, (float*)p, (int64_t)count, c->ipc, seq, c->dIpcErr, c->ipc_wait_ticks);
    HIPCHK(c, hipGetLastError());
    ++c->ipc_calls;
    return PMF_OK;
  }
  if (c->host_ar) {
    ++c->host_calls;
    const size_t bytes = count * (f64 ? sizeof(double) : sizeof(float));
    c->ar_buf.resize(bytes);
    HIPCHK(c, hipMemcpyAsync(c->ar_buf.data(), p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->host_ar(c->host_ar_user, c->ar_buf.data(), (int64_t)count, f64 ? 1 : 0) != 0)
      return fail(c, PMF_ENCCL, "the host all-reduce callback reported a failure");
    HIPCHK(c, hipMemcpyAsync(p, c->ar_buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PMF_OK;
  }
  if (c->comm) {
    ++c->rccl_calls;
    NCCLCHK(c, ncclAllReduce(p, p, count, f64 ? ncclDouble : ncclFloat, ncclSum, c->comm, c->stream));
  }
  return PMF_OK;
}

bool multi_rank(const pmf_ctx* c) { return c->comm != nullptr || c->host_ar != nullptr || c->ipc.nranks > 1; }

// a peer that never raised its flags (k_ipc_allreduce gave up after ipc_wait_ticks of polling: 30 s in the loops, 2 s in the self-test)
int ipc_check(pmf_ctx* c) {
  if (c->ipc.nranks <= 1 || !c->dIpcErr) return PMF_OK;
  int e = 0;
  HIPCHK(c, hipMemcpyAsync(&e, c->dIpcErr, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (e) {
    HIPCHK(c, hipMemsetAsync(c->dIpcErr, 0, sizeof(int), c->stream));
    return fail(c, PMF_ENCCL, "one-shot all-reduce: a peer rank did not arrive (its flags were not raised within the polling limit)");
  }
  return PMF_OK;
}

// The per-iteration collective: (W^T V | W^T W) summed over the ranks.  With pmf_profile_enable its launches are bracketed by
// HIP events of their own (pmf_collective_ms: what the exchange costs an iteration at N > 1, next to the dominant kernel).
int allreduce_ps(pmf_ctx* c) {
  // (timed only where the sum is a device operation on the stream: the one-shot kernel or ncclAllReduce -- a payload that
  //  falls back to the blocking host round trip has nothing for HIP events to bracket)
  const bool on_stream = (c->ipc.nranks > 1 && (size_t)ps_elems(c) * sizeof(float) <= PMF_IPC_MAX_BYTES) || (!c->host_ar && c->comm);
  const bool timed = c->profile && multi_rank(c) && on_stream && (c->coll_seen++ % c->stat.every == 0);   // sampled like the kernel's
  if (timed) {
    if (c->coll_used + 2 > c->coll_ev.size())
      for (int q = 0; q < 2; ++q) { hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) c->coll_ev.push_back(e); }
    if (c->coll_used + 2 <= c->coll_ev.size()) (void)hipEventRecord(c->coll_ev[c->coll_used], c->stream);
  }
  const int rc = allreduce_sum(c, c->dPS, (size_t)ps_elems(c), false);
  if (timed && c->coll_used + 2 <= c->coll_ev.size()) {
    (void)hipEventRecord(c->coll_ev[c->coll_used + 1], c->stream);
    c->coll_used += 2;
  }
  return rc;
}

}  // namespace
