// pmf_host_algos.h -- the table of algorithms: what pmf_ctx_create, pmf_update_w / pmf_update_h, pmf_frobenius, pmf_factorize and
// pmf_stream_begin need to know about a class family, one row per PMF_ALGO_* number.  A new class registers here.
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

struct Operands { bool v, w, h; };   // what need() asks for

// what pmf_factorize(compute_w, compute_h) reads before it writes
Operands loop_reads_all(bool, bool) { return {true, true, true}; }
Operands loop_reads_unwritten(bool cw, bool ch) { return {true, !cw, !ch}; }        // either step writes its factor from scratch
Operands loop_reads_aa(bool cw, bool ch) { return {true, !cw, cw || !ch}; }         // the W step reads H, the H step W

// ---- the limits of a family for pmf_ctx_create: the message of the first one that (rows, cols, bases) exceed, or null ----------
// C = V^T V is n x n float64 (128 MiB at the limit); the k x k factors on one float64 MFMA tile row
const char* cnmf_limits(int64_t, int64_t n, int k) {
  if (n > 4096) return "CNMF: n (samples) > 4096 is not supported by this build";
  if (k > 128) return "CNMF: num_bases > 128 is not supported by this build";
  if (k > n) return "CNMF: num_bases > n (the k-means initialisation samples num_bases columns)";
  return nullptr;
}
// k_cluster_pass holds one column's distances to all bases in the registers of four lanes
const char* cluster_limits(int64_t, int64_t, int k) {
  return k > 128 ? "Kmeans / Cmeans: num_bases > 128 is not supported by this build" : nullptr;
}
// the H step's QPs run on the kernels of num_bases <= 64; k_sivm_pass stages one column of V in LDS
const char* sivm_limits(int64_t m, int64_t, int k) {
  if (k > 64) return "SIVM: num_bases > 64 is not supported by this build";
  if (m > PMF_SIVM_MAX_M) return "SIVM: data_dimension > 16384 is not supported by this build";
  return nullptr;
}
// the H step is SIVM's; a base's corral holds an affinely independent set of data columns: at most min(m + 1, n)
const char* aa_limits(int64_t m, int64_t n, int k) {
  if (k > 64) return "AA: num_bases > 64 is not supported by this build";
  if (std::min<int64_t>(m + 1, n) > PMF_AA_MAX_CORRAL) return "AA: min(data_dimension + 1, num_samples) > 128 (the corral bound) is not supported by this build";
  return nullptr;
}
// the Gram matrix on the short side goes through the full Jacobi solver; U and V travel as bases of the product paths
const char* pca_limits(int64_t m, int64_t n, int k) {
  if (std::min<int64_t>(m, n) > PMF_SVD_MAX_RANK) return "PCA / SVD: min(rows, cols) > 2432 is not supported by this build";
  if (k < std::min<int64_t>(m, n)) return "PCA / SVD: the context's base count must be at least min(rows, cols) (the largest possible rank)";
  return nullptr;
}
// the sampled rows and columns are two 64-wide tiles of k_prod_f64 and one 128-wide block of W and H
const char* cur_limits(int64_t, int64_t, int k) {
  return k > PMF_CUR_MAX_RANK ? "CUR / CMD: more than 128 sampled rows or columns are not supported by this build" : nullptr;
}
// the staged operand [B' | Q] of k_greedy_pass has 2 k - 1 <= 127 columns; the short side goes through the Jacobi solver
const char* greedy_limits(int64_t m, int64_t n, int k) {
  if (k > PMF_GREEDY_MAX_BASES) return "GREEDY: num_bases > 64 is not supported by this build";
  if (std::min<int64_t>(m, n) > PMF_SVD_MAX_RANK) return "GREEDY: min(rows, cols) > 2432 is not supported by this build";
  return nullptr;
}
// NMFALS / NMFNNLS beyond 128 bases solve one variable at a time (k_nnqp_big) and stay at 1 024
const char* nmfals_limits(int64_t, int64_t, int k) {
  return k > 1024 ? "num_bases > 1024 is not supported for NMFALS / NMFNNLS by this build" : nullptr;
}

int nmf_frobenius(pmf_ctx* c, double* out) {
  PMFCHK(do_frobenius(c, out));
  return ipc_check(c);
}
int cnmf_frobenius(pmf_ctx* c, double* out) {
  PMFCHK(cnmf_ready(c));
  return cnmf_error(c, false, out);
}

struct AlgoRow {
  const char* family;          // the name in messages; null: the number is not assigned
  const char* path;            // pmf_path_name; null: pmf_ctx_create computes the name from the shape
  bool nmf_family;             // the steps of pmf_host_nmf*.h / pmf_host_snmf.h: NmfLoopSteps in pmf_factorize, ipc_check and check_singular behind a step
  bool one_rank;               // pmf_ctx_create refuses nranks > 1
  bool dense_w, dense_h;       // the step refuses CSR data
  bool streamable;             // pmf_stream_*
  bool run_once;               // both steps give the same bits every time: pmf_factorize's iterations behind the first repeat its result
  Operands reads_w, reads_h;   // what pmf_update_w / pmf_update_h need
  Operands (*loop_reads)(bool cw, bool ch);
  int (*update_w)(pmf_ctx*);   // null steps: the entry points refuse, naming `instead`
  int (*update_h)(pmf_ctx*);
  int (*frobenius)(pmf_ctx*, double*);    // pmf_frobenius
  int (*loop_error)(pmf_ctx*, double*);   // the error behind an iteration of pmf_factorize
  const char* instead;
  const char* (*limits)(int64_t m, int64_t n, int k);
};

constexpr Operands kV{true, false, false}, kVW{true, true, false}, kVH{true, false, true}, kVWH{true, true, true};

// CNMF's hooks are no-ops and its loop free-runs in Gram space (CnmfLoopSteps): its row carries no steps.
// Kmeans' W step reads the assignment and keeps the columns of centres with < 2 members (kmeans.py:82-87), Cmeans' reads H
// (cmeans.py:83-86); SIVM's, GREEDY's and PCA's read the data alone (sivm.py:145-201, greedy.py:88-170, pca.py:93-108); AA's reads
// the data and H (W_hat = data pinv(H), aa.py:113-134).  The reference's RNMF keeps S, an in-memory array of data's shape
// (rnmf.py:94-98): not streamable.
constexpr AlgoRow kAlgos[] = {
    // family              path              nmf    1rank  denW   denH   stream once   reads_w reads_h loop_reads            update_w          update_h          frobenius         loop_error        instead  limits
    {"NMF",              nullptr,          true,  false, false, false, true,  false, kVWH, kVWH, loop_reads_all,       do_update_w,      do_update_h,      nmf_frobenius,    nullptr,          nullptr, nullptr},
    {"NMFALS",           nullptr,          true,  false, false, false, true,  false, kVWH, kVWH, loop_reads_all,       do_update_w,      do_update_h,      nmf_frobenius,    nullptr,          nullptr, nmfals_limits},
    {"SNMF",             nullptr,          true,  false, false, false, true,  false, kVWH, kVWH, loop_reads_all,       do_update_w,      do_update_h,      nmf_frobenius,    nullptr,          nullptr, nullptr},
    {"BNMF",             nullptr,          true,  false, false, false, true,  false, kVWH, kVWH, loop_reads_all,       do_update_w,      do_update_h,      nmf_frobenius,    nullptr,          nullptr, nullptr},
    {"RNMF",             nullptr,          true,  false, false, false, false, false, kVWH, kVWH, loop_reads_all,       do_update_w,      do_update_h,      nmf_frobenius,    nullptr,          nullptr, nullptr},
    {"CNMF",             "cnmf_gram",      false, true,  false, false, false, false, kVWH, kVWH, loop_reads_all,       nullptr,          nullptr,          cnmf_frobenius,   nullptr,          nullptr, cnmf_limits},
    {"Kmeans / Cmeans",  "cluster_panels", false, true,  false, false, false, false, kVW,  kVW,  loop_reads_all,       cluster_update_w, cluster_update_h, cluster_frobenius, cluster_error,   nullptr, cluster_limits},
    {},
    {"Kmeans / Cmeans",  "cluster_panels", false, true,  false, false, false, false, kVH,  kVW,  loop_reads_all,       cluster_update_w, cluster_update_h, cluster_frobenius, cluster_error,   nullptr, cluster_limits},
    {},
    {"SIVM",             "sivm_panels",    false, true,  true,  false, false, false, kV,   kVW,  loop_reads_unwritten, sivm_update_w,    sivm_update_h,    frobenius_direct, frobenius_direct, nullptr, sivm_limits},
    {"AA",               "aa_pricing",     false, true,  true,  true,  false, false, kVH,  kVW,  loop_reads_aa,        aa_update_w,      aa_update_h,      frobenius_direct, frobenius_direct, nullptr, aa_limits},
    {"PCA / SVD",        "svd_gram_f64",   false, true,  false, false, false, false, kV,   kVW,  loop_reads_unwritten, pca_update_w,     pca_update_h,     pca_error,        pca_error,        nullptr, pca_limits},
    {},
    {"CUR / CMD",        "cur_cross_f64",  false, true,  false, false, false, false, kV,   kV,   loop_reads_all,       nullptr,          nullptr,          frobenius_direct, nullptr,          "pmf_cur_compute is the decomposition", cur_limits},
    {"GREEDY",           "greedy_panels",  false, true,  false, false, false, true,  kV,   kVW,  loop_reads_unwritten, greedy_update_w,  greedy_update_h,  greedy_error,     greedy_error,     nullptr, greedy_limits},
};
constexpr int kAlgoCount = (int)(sizeof(kAlgos) / sizeof(kAlgos[0]));
static_assert(kAlgoCount == PMF_ALGO_GREEDY + 1, "one row per PMF_ALGO_* number");

const AlgoRow& algo_row(const pmf_ctx* c) { return kAlgos[c->algo]; }

// a family without a W step, an H step or an iteration: what = "W step", "H step", "iteration"
int refuse_step(pmf_ctx* c, const char* what) {
  const AlgoRow& a = algo_row(c);
  return fail(c, PMF_EINVAL, std::string(a.family) + ": no " + what + " (" + a.instead + ")");
}

// pmf_factorize for the families whose iteration is their W step, then their H step (nmf.py:183-187), with no free-running form
struct TableLoopSteps {
  const AlgoRow& a;
  bool cw, ch;
  double f = 0.0;
  int iterate(pmf_ctx* c, int i) {
    if (a.run_once && i > 0) return PMF_OK;
    if (cw) PMFCHK(a.update_w(c));
    if (ch) PMFCHK(a.update_h(c));
    return PMF_OK;
  }
  int error(pmf_ctx* c, int i, double* out) {
    if (!a.run_once || i == 0) PMFCHK(a.loop_error(c, &f));
    *out = f;
    return PMF_OK;
  }
  bool may_free_run(const pmf_ctx*, int, double) const { return false; }
  int enqueue(pmf_ctx* c, int, int, int, double) { return fail(c, PMF_EINVAL, "no free-running loop");   /* (never called: may_free_run is false) */ }
  void rewind(pmf_ctx*, int, int) {}
  int close(pmf_ctx*) { return PMF_OK; }
};

}  // namespace
