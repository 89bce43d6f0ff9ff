// pmf_host_factorize.h -- NMF / BNMF / RNMF / SNMF / NMFALS: the steps that pmf_factorize hands to the loop (pmf_host_loop.h)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// ---- what a stop inside a chunk takes back: the launches behind it were no-ops, but the host counted them as enqueued ----
// The FOLDED exchanges behind the stop neither pushed nor waited (k_reduce_slabs_tiles / k_nmf_h_gram return on the
// flag), on every rank alike (H, and with it the stop, is bit-identical across ranks): take their sequence numbers back,
// so that the next exchange that really runs is the successor of the last one that did.  Counting the skipped ones
// broke the two-slot invariant of pmf_ipc.h (a rank is at most one exchange ahead of a peer BECAUSE it needs that
// peer's flags of exchange s + 1 before it can push s + 2 into the slot of s): after an odd number of skipped exchanges
// the next push could land in a slot a slower peer was still adding up (round-5 advisor).  k_ipc_allreduce launches
// run whatever the flag says, so a chunk that used those keeps its count.
void rewind_exchange_count(pmf_ctx* c, unsigned ipc_seq0, long long fold_calls0, unsigned seq_at_stop) {
  if (c->fold_calls - fold_calls0 != (long long)(c->ipc_seq - ipc_seq0) || c->ipc_seq == ipc_seq0) return;
  const long long skipped = (long long)(c->ipc_seq - seq_at_stop);
  c->ipc_seq = seq_at_stop;
  c->ipc_calls -= skipped; c->fold_calls -= skipped;
}

// BNMF: every H step scales the penalty weights (bnmf.py:84-85), and only `ran` H steps of the chunk really ran
void rewind_bnmf_schedule(pmf_ctx* c, double lamb_w0, double lamb_h0, int ran) {
  c->lamb_w = lamb_w0; c->lamb_h = lamb_h0;
  for (int q = 0; q < ran; ++q) { c->lamb_w *= 1.1; c->lamb_h *= 1.1; }
}

// the host-side picture of where G lives was advanced by the no-ops: put it back to what iteration s_it's H step (the
// last that ran) left
void rewind_gram_partials(pmf_ctx* c, int s_it, int niter) {
  const bool part = s_it + 1 < niter && !c->fused8;
  c->g_parts = part ? std::min(c->np / 64, PMF_HGRAM_MAX_WGS) : 0;
}

// the trace terms on the device are those of a no-op; with several ranks the all-reduces behind the stop still ran, on
// the stale (P | S): it no longer belongs to W
void drop_sums_behind_stop(pmf_ctx* c) {
  c->trace_ready = false;
  if (multi_rank(c)) c->ps_valid = false;
}

struct NmfLoopSteps {
  bool cw = false, ch = false;
  int niter = 0;
  bool fused = false;          // update_w + update_h in one pass over V
  bool h_only = false;         // the fixed-basis loop (compute_w = False, nmf.py:56-65: coefficients for an existing basis):
                               // (W^T V | W^T W) is formed once, every further iteration is the H-step kernel alone
  bool gram = false;           // SNMF with both updates on: the loop runs in Gram space (snmf_gram_iteration), W materialised at the end
  bool can_free_run = false;   // NMF, BNMF, SNMF on the fused kernel (or in Gram space, or h_only) with the error on
  // where the chunk under way started
  double lamb_w0 = 0.0, lamb_h0 = 0.0;
  unsigned ipc_seq0 = 0; long long fold_calls0 = 0;
  unsigned seq_after[kLoopChunk];   // the exchange counter behind iteration i + j

  bool partials_ok(const pmf_ctx* c, int next) const {   // the next consumer of G is the one-pass kernel
    return (c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_BNMF) && next < niter && !c->fused8;
  }

  int iterate(pmf_ctx* c, int i) {
    if (gram) { PMFCHK(ensure_vgram(c)); return snmf_gram_iteration(c); }   // SNMF on k x n sized data (C = V^T V, formed once per V)
    if (cw && ch && c->algo == PMF_ALGO_SNMF && csr_fused_ok(c)) return snmf_csr_fused_iteration(c);   // CSR: one pass over the rows
    if (fused) {                                          // update_w + update_h, one pass over V
      c->gram_partial_ok = partials_ok(c, i + 1);
      return c->algo == PMF_ALGO_SNMF ? snmf_fused_iteration(c) : nmf_fused_iteration(c);
    }
    if (cw) PMFCHK(do_update_w(c));                       // nmf.py:183-184
    if (ch) PMFCHK(do_update_h(c));                       // nmf.py:186-187
    return PMF_OK;
  }

  int error(pmf_ctx* c, int, double* out) {
    if (c->algo == PMF_ALGO_RNMF && ch) {                 // update_s already summed (V - W H)^2
      HIPCHK(c, hipStreamSynchronize(c->stream));
      *out = std::sqrt(c->rnmf_err2);
      return PMF_OK;
    }
    return do_frobenius(c, out);
  }

  bool may_free_run(const pmf_ctx* c, int i, double f) const {
    return can_free_run && i + 1 >= 1 /* iterations in the ordinary form first */ && niter - (i + 1) >= 2 && c->vnorm_valid && f * f > 1e-2 * c->vnorm2;
  }

  int enqueue(pmf_ctx* c, int i, int j, int chunk, double conv_eps) {
    if (j == 0) { lamb_w0 = c->lamb_w; lamb_h0 = c->lamb_h; ipc_seq0 = c->ipc_seq; fold_calls0 = c->fold_calls; }
    c->gram_partial_ok = partials_ok(c, i + j + 1);
    int lrc = h_only ? ensure_ps(c)                       // current since the first iteration (W is fixed)
              : gram ? snmf_gram_iteration(c) : c->algo == PMF_ALGO_SNMF ? snmf_fused_iteration(c) : nmf_fused_iteration(c);
    if (h_only && lrc == PMF_OK) lrc = h_step_from_ps(c);
    const double* tt = c->dScal + 2;                      // k_nmf_h_gram left <P,H>, <S,G> there ...
    int ntt = 1;
    if (lrc == PMF_OK && c->trace_ready && c->trace_parts > 0) { tt = c->dT1part; ntt = c->trace_parts; }   // ... or as pairs
    if (lrc == PMF_OK && !c->trace_ready) {               // SNMF: the H-step kernel does not form them
      const int nb = c->np / 16;
      lrc = launch_trace_terms(c);
      hipLaunchKernelGGL(k_sum_pairs_f64, dim3(1), dim3(256), 0, c->stream, c->dPart, nb, c->dScal);
      tt = c->dScal;
    }
    // the next launch of the chunk is a one-pass kernel: it evaluates this iteration's error and the
    // convergence test in its prologue (FusedCtl) -- no launch of its own for them
    const bool fold = fused && !c->fused8 && !h_only && j + 1 < chunk && c->algo != PMF_ALGO_SNMF;
    if (lrc == PMF_OK && fold) {
      c->conv_iter = i + j; c->conv_tt = tt; c->conv_ntt = ntt; c->conv_eps = conv_eps;
    } else {
      c->conv_iter = -1;                                  // (nothing pending behind the chunk's last iteration, or behind an error)
      if (lrc == PMF_OK) lrc = launch_conv_check(c, tt, ntt, c->vnorm2, conv_eps, i + j);
    }
    seq_after[j] = c->ipc_seq;
    return lrc;
  }

  void rewind(pmf_ctx* c, int i, int s_it) {
    rewind_exchange_count(c, ipc_seq0, fold_calls0, seq_after[s_it - i]);
    if (c->algo == PMF_ALGO_BNMF) rewind_bnmf_schedule(c, lamb_w0, lamb_h0, s_it - i + 1);
    if (c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_BNMF) rewind_gram_partials(c, s_it, niter);
    drop_sums_behind_stop(c);
  }

  int close(pmf_ctx* c) {
    c->want_trace = c->fixed_h_loop = c->gram_partial_ok = false;
    PMFCHK(nmf_csr_sync_h(c));   // NMF on CSR data: dH follows the working copy H^T
    return materialize_w(c);     // Gram-space SNMF loop: W = V M once
  }
};

// Which form of the iteration this call runs: fills the steps and raises the context's loop flags (close() clears them)
NmfLoopSteps nmf_loop_steps(pmf_ctx* c, int niter, bool cw, bool ch, bool ce) {
  NmfLoopSteps s;
  s.cw = cw; s.ch = ch; s.niter = niter;
  c->want_trace = ce;
  c->fixed_h_loop = cw && !ch && niter > 1 && c->algo == PMF_ALGO_NMF;
  s.fused = cw && ch && c->fused_wgs > 0 && !use_csr(c) &&
            (c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_SNMF || c->algo == PMF_ALGO_BNMF || c->algo == PMF_ALGO_RNMF);
  s.h_only = !cw && ch && ce && c->nb == 1 && !use_csr(c) && (c->algo == PMF_ALGO_NMF || c->algo == PMF_ALGO_BNMF);
  s.gram = cw && ch && snmf_gram_ok(c, niter);
  choose_stat_site(c, s.gram);
  // (a host transport blocks on the host in every iteration -- nothing to free-run -- unless the per-iteration payload
  //  (P | S) fits the one-shot IPC all-reduce in front of it)
  s.can_free_run = ((((s.fused && c->algo != PMF_ALGO_RNMF) || (s.gram && !use_csr(c) && c->nb == 1)) && ce) || s.h_only) &&
                   !(c->host_ar && !(c->ipc.nranks > 1 && (size_t)ps_elems(c) * sizeof(float) <= PMF_IPC_MAX_BYTES));
  return s;
}

// every early (error) return of pmf_factorize leaves no pipelined W = V M write in flight on the side stream: a caller that
// then re-uploads W must not see the stale product land on top of it
struct WPipeGuard {
  pmf_ctx* c; bool ok = false;
  ~WPipeGuard() {
    if (ok || !c->w_stream) return;
    (void)hipStreamSynchronize(c->w_stream);
    c->ev_w_pending[0] = c->ev_w_pending[1] = false;
  }
};

}  // namespace
