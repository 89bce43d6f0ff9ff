// pmf_host_loop.h -- the iteration loop of pmf_factorize, once for every class family (kernel: pmf_small.h: k_conv_check)
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

constexpr int kLoopChunk = 32;   // iterations enqueued back to back between two reads of the stop flag

// The error of iteration `it` from the ntt pairs of trace terms at tt, the convergence test of nmf.py:134-139 on it and the
// stop flag (dStop[0]: 1 converged, 2 the trace identity cancels; dStop[1]: where), on the device behind that iteration
int launch_conv_check(pmf_ctx* c, const double* tt, int ntt, double vnorm2, double eps, int it) {
  hipLaunchKernelGGL(k_conv_check, dim3(1), dim3(64), 0, c->stream, tt, ntt, vnorm2, eps, (double)c->n, it, c->dFerr, c->dStop);
  if (hipGetLastError() != hipSuccess) return fail(c, PMF_EHIP, "k_conv_check launch failed");
  return PMF_OK;
}

// The loop of nmf.py:182-202 for every class.  A class family hands in its own steps (a struct, resolved at compile time:
// the enqueue loop is on the critical path of a 60 us iteration):
//   iterate(c, i)                 ordinary iteration i
//   error(c, i, &f)               the error behind it
//   may_free_run(c, i, f)         may the loop hand over to the device after iteration i with error f?
//   enqueue(c, i, j, chunk, eps)  free-running iteration i + j of a chunk that starts at i, with its convergence check
//   rewind(c, i, s_it)            the chunk from i stopped at s_it: put the host's picture back to what really ran
//   close(c)                      what ends the timed region of the loop
// Free-running form: after an ordinary iteration far from the cancellation threshold, chunks of iterations are enqueued back
// to back; the error and the convergence test run on the device and a raised stop flag turns every later launch of the chunk
// into a no-op, so the results are those of the ordinary loop while the host reads back once per chunk, not once per iteration.
template <class Steps>
int factorize_loop(pmf_ctx* c, Steps& s, int niter, bool ce, double conv_eps, double* ferr, int32_t* iters_done, int32_t* converged_at) {
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  int done = 0;
  bool free_run = false;
  for (int i = 0; i < niter; ++i) {                       // nmf.py:182
    if (c->abort_flag.load(std::memory_order_relaxed) != 0) break;   // pmf_abort: the caller discards this run (iters_done says how far it got)
    if (free_run) {
      const int chunk = std::min(kLoopChunk, niter - i);
      c->stop_arg = c->dStop;
      int lrc = PMF_OK;
      for (int j = 0; j < chunk && lrc == PMF_OK; ++j) lrc = s.enqueue(c, i, j, chunk, conv_eps);
      c->stop_arg = nullptr;
      PMFCHK(lrc);
      int hstop[2] = {0, -1};
      HIPCHK(c, hipMemcpyAsync(hstop, c->dStop, sizeof(hstop), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(ferr + i, c->dFerr + i, (size_t)chunk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (hstop[0] == 0) { done += chunk; i += chunk - 1; continue; }   // the whole chunk ran
      // iterations i .. hstop[1] ran, the rest of the chunk were no-ops
      const int s_it = hstop[1];
      done += s_it - i + 1;
      s.rewind(c, i, s_it);
      if (hstop[0] == 1) {                                // nmf.py:198-202
        if (converged_at) *converged_at = s_it;
        break;
      }
      // the trace identity cancels at iteration s_it: evaluate it directly and go on in the ordinary form
      free_run = false;
      i = s_it;
      PMFCHK(frobenius_direct(c, &ferr[i]));
    } else {
      PMFCHK(s.iterate(c, i));                            // nmf.py:183-187
      ++done;
      if (ce) PMFCHK(s.error(c, i, &ferr[i]));            // nmf.py:189-190
    }
    if (ce && i > 1) {                                    // nmf.py:198
      const double derr = std::fabs(ferr[i] - ferr[i - 1]) / (double)c->n;   // nmf.py:135
      if (derr < conv_eps) {                              // nmf.py:136
        if (converged_at) *converged_at = i;              // caller: ferr = ferr[:i] (nmf.py:201)
        break;
      }
    }
    if (ce && !free_run && s.may_free_run(c, i, ferr[i])) {
      // far from the cancellation threshold: hand the history to the device and let it run
      PMFCHK(dgrow(c, &c->dFerr, &c->ferr_cap, niter));
      if (!c->dStop) PMFCHK(dalloc(c, &c->dStop, 2));
      HIPCHK(c, hipMemcpyAsync(c->dFerr, ferr, (size_t)(i + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemsetAsync(c->dStop, 0, 2 * sizeof(int), c->stream));
      free_run = true;
    }
  }
  PMFCHK(s.close(c));            // inside the timed loop region
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->last_loop_ms = ms;
  if (ce) for (int q = done; q < niter; ++q) ferr[q] = 0.0;   // as np.zeros(niter) leaves them (nmf.py:179-180)
  if (iters_done) *iters_done = done;
  return PMF_OK;
}

}  // namespace
