// aggregate_rows.h -- what the aggregation kernels share (block_aggregate.hip: sampled COO blocks, float atomics;
// csr_aggregate.hip: whole CSR rows, one owner per row): the row types a lane loads, and the argument checks of their
// launch paths.
#pragma once
#include <hip/hip_fp16.h>

#include "fgnn_device.h"

namespace fgnn {

// What a lane loads of a row per slot -- the kernels' Row parameter: float (fp32 rows), __half2 (fp16 rows whose base
// and stride are 4-byte aligned: two columns per lane, so that a wave's load still covers 256 contiguous bytes) or
// __half (fp16 rows with an odd base, stride or dim: one column per lane, correct at half the width).
template <typename Row> inline constexpr int kRowCols = 1;
template <> inline constexpr int kRowCols<__half2> = 2;
template <typename Row> __device__ __forceinline__ Row row_zero() { return Row(0.0f); }
template <> __device__ __forceinline__ __half2 row_zero<__half2>() { return __half2(__half(0.0f), __half(0.0f)); }
__device__ __forceinline__ float row_col(float r, int) { return r; }
__device__ __forceinline__ float row_col(__half r, int) { return __half2float(r); }
__device__ __forceinline__ float row_col(__half2 r, int j) { return j ? __high2float(r) : __low2float(r); }

// fp16 rows are read two columns per lane unless the base, the stride or dim is odd
inline bool half_rows_paired(const void *h, size_t h_ld, size_t dim) {
  return ((reinterpret_cast<uintptr_t>(h) & 3u) | (h_ld & 1u) | (dim & 1u)) == 0;
}

// The checks every aggregation entry point makes on its matrices, weights and scalings before any launch: null h / out,
// dim == 0, a stride below dim, sizes beyond 32 bits, modes out of range, a mode without its degree vector
// (dst_deg_implied: the caller has another source for the destination degree), pointers that are not 4-byte aligned
// (h_f16: h holds binary16 rows and need only be 2-byte aligned).
inline bool aggregate_args_ok(bool h_f16, const void *h, size_t h_ld, size_t dim, const float *out, size_t out_ld,
                              const float *edge_weight, const float *src_deg, int src_mode, const float *dst_deg,
                              int dst_mode, bool dst_deg_implied = false) {
  if (!h || !out || dim == 0 || !fits_u32(dim) || h_ld < dim || !fits_u32(h_ld) || out_ld < dim || !fits_u32(out_ld))
    return false;
  if (src_mode < 0 || src_mode > 2 || dst_mode < 0 || dst_mode > 2 || (src_mode && !src_deg) ||
      (dst_mode && !dst_deg && !dst_deg_implied))
    return false;
  return (h_f16 ? (reinterpret_cast<uintptr_t>(h) & 1u) == 0 : float_aligned(h)) && float_aligned(out) &&
         float_aligned(edge_weight) && float_aligned(src_deg) && float_aligned(dst_deg);
}

}  // namespace fgnn
