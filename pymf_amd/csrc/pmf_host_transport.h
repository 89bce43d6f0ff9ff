// pmf_host_transport.h -- host <-> device transport: stage_reserve, upload_rows, download_rows
// Host code of libpymf_hip.so: included by pmf_api.hip (the translation unit) in this order, nothing else includes it.
#pragma once

namespace {

// Staging area for the host <-> device transport (grown on demand, at most kStageBytes at a time)
constexpr size_t kStageBytes = (size_t)256 << 20;
int stage_reserve(pmf_ctx* c, size_t bytes) {
  if (c->stage_cap >= bytes) return PMF_OK;
  bytes = std::max<size_t>(bytes, (size_t)4 << 20);          // (H and other k x n sized arrays: one allocation serves them all)
  if (c->dStage) HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stage_cap = 0;
  PMFCHK(dfree(c, &c->dStage));
  PMFCHK(dalloc_raw(c, &c->dStage, bytes));       // (every byte read from it has been written first: no zero fill)
  c->stage_cap = bytes;
  return PMF_OK;
}

// Host [rows][cols] (leading dimension sld, float32 or float64) -> device [rows][dld] float32, zero padded.  Contiguous host
// rows go up as they are in ONE hipMemcpyAsync per chunk (56 GB/s from pageable memory; hipMemcpy2DAsync: 17) and are padded /
// rounded by k_unpack_rows on the device; only a host array with a leading dimension of its own takes the pitched copy.
template <typename T>
int upload_rows(pmf_ctx* c, float* dst, int64_t dld, const T* src, int64_t sld, int64_t rows, int64_t cols) {
  constexpr bool f32 = sizeof(T) == sizeof(float);
  if (rows <= 0 || cols <= 0) return PMF_OK;
  if (f32 && sld == cols && dld == cols) {                    // nothing to pad, nothing to round
    HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)rows * cols * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PMF_OK;
  }
  if (f32 && sld != cols) {                                   // a pitched host array
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)dld * sizeof(float), src, (size_t)sld * sizeof(float),
                               (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PMF_OK;
  }
  const int64_t chunk_rows = std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t)(kStageBytes / ((size_t)cols * sizeof(T)))));
  PMFCHK(stage_reserve(c, (size_t)chunk_rows * cols * sizeof(T)));
  for (int64_t r0 = 0; r0 < rows; r0 += chunk_rows) {
    const int64_t nr = std::min(chunk_rows, rows - r0);
    if (sld == cols)
      HIPCHK(c, hipMemcpyAsync(c->dStage, src + r0 * sld, (size_t)nr * cols * sizeof(T), hipMemcpyHostToDevice, c->stream));
    else
      HIPCHK(c, hipMemcpy2DAsync(c->dStage, (size_t)cols * sizeof(T), src + r0 * sld, (size_t)sld * sizeof(T), (size_t)cols * sizeof(T),
                                 (size_t)nr, hipMemcpyHostToDevice, c->stream));
    const unsigned grid = (unsigned)std::min<int64_t>((nr * dld + 255) / 256, 8192);
    hipLaunchKernelGGL((k_unpack_rows<T>), dim3(grid), dim3(256), 0, c->stream, reinterpret_cast<const T*>(c->dStage), nr, cols, dst + r0 * dld, dld);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

int upload_padded(pmf_ctx* c, float* dst, int64_t dld, const float* src, int64_t sld, int64_t rows, int64_t cols) {
  return upload_rows<float>(c, dst, dld, src, sld, rows, cols);
}

// device [rows][sld] float32 -> host [rows][cols] contiguous float32 / float64 (the rounding to the host array's float64 on
// the device: np.copyto(float64, float32) of a 1 048 576 x 64 W is 0.1 s in one host thread)
template <typename T>
int download_rows(pmf_ctx* c, T* dst, const float* src, int64_t sld, int64_t rows, int64_t cols) {
  constexpr bool f32 = sizeof(T) == sizeof(float);
  if (rows <= 0 || cols <= 0) return PMF_OK;
  if (f32 && sld == cols) {
    HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)rows * cols * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PMF_OK;
  }
  const int64_t chunk_rows = std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t)(kStageBytes / ((size_t)cols * sizeof(T)))));
  PMFCHK(stage_reserve(c, (size_t)chunk_rows * cols * sizeof(T)));
  for (int64_t r0 = 0; r0 < rows; r0 += chunk_rows) {
    const int64_t nr = std::min(chunk_rows, rows - r0);
    const unsigned grid = (unsigned)std::min<int64_t>((nr * cols + 255) / 256, 8192);
    hipLaunchKernelGGL((k_pack_rows<T>), dim3(grid), dim3(256), 0, c->stream, src + r0 * sld, sld, nr, cols, reinterpret_cast<T*>(c->dStage));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(dst + r0 * cols, c->dStage, (size_t)nr * cols * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // the staging area is reused by the next chunk
  }
  return PMF_OK;
}

int download_padded(pmf_ctx* c, float* dst, int64_t dld, const float* src, int64_t sld, int64_t rows, int64_t cols) {
  if (dld == cols) return download_rows<float>(c, dst, src, sld, rows, cols);
  HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)dld * sizeof(float), src, (size_t)sld * sizeof(float),
                             (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PMF_OK;
}

}  // namespace
