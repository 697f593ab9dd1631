// q8_rows.h -- what the kernels over an 8-bit feature store share (q8_rows.hip): the row format, the argument checks of
// their launch paths, and the per-lane pieces -- sixteen codes of one 16-byte load into sixteen fp32 accumulators.
// A row of D columns occupies S = round_up(D, 16) + 16 bytes:
//     [0, D)         codes q_j, unsigned 8-bit
//     [D, S - 16)    zero
//     [S - 16, S)    the header: scale (fp32), lo (fp32), eight zero bytes
// and stands for x^_j = lo + scale * q_j.  S is a multiple of 16: tables, caches and batches of such rows move through
// the gather's 16-byte vector path as FGNN_U8 rows of S elements, and a lane's one dwordx4 load holds sixteen codes.
#pragma once
#include "aggregate_rows.h"

namespace fgnn {

constexpr uint32_t kQ8Group = 16;        // lanes that own one edge's row
constexpr uint32_t kQ8LaneBytes = 16;    // one dwordx4 per lane: sixteen codes
constexpr uint32_t kQ8PassBytes = kQ8Group * kQ8LaneBytes;  // 256 contiguous bytes of a row per group load
constexpr uint32_t kQ8Groups = kWave / kQ8Group;            // four edges' rows per wave instruction

inline size_t q8_row_bytes(size_t dim) { return ((dim + 15) & ~(size_t)15) + 16; }

// h: q8 rows -- a 16-byte aligned base and a row stride in bytes that is a multiple of 16 and holds a row
inline bool q8_rows_ok(const void *h, size_t h_ld, size_t dim) {
  return h && dim != 0 && fits_u32(dim) && fits_u32(h_ld) && h_ld >= q8_row_bytes(dim) && h_ld % 16 == 0 &&
         (reinterpret_cast<uintptr_t>(h) & 15u) == 0;
}

// The checks of the q8 aggregation entry points before any launch: aggregate_args_ok's, with h held to q8_rows_ok
// (aggregate_args_ok's own h_ld >= dim follows from it: a row is longer than its codes; its h_f16 flag is set only to
// keep it from asking h for fp32 alignment -- the 16-byte alignment q8 rows need is q8_rows_ok's).
inline bool q8_aggregate_args_ok(const void *h, size_t h_ld, size_t dim, const float *out, size_t out_ld,
                                 const float *edge_weight, const float *src_deg, int src_mode, const float *dst_deg,
                                 int dst_mode, bool dst_deg_implied = false) {
  return q8_rows_ok(h, h_ld, dim) && aggregate_args_ok(true, h, h_ld, dim, out, out_ld, edge_weight, src_deg, src_mode,
                                                        dst_deg, dst_mode, dst_deg_implied);
}

// byte b of a dword as fp32: the byte-to-float conversions (v_cvt_f32_ubyte0..3), no sign extension
__device__ __forceinline__ float q8_code(uint32_t word, int b) { return (float)((word >> (8 * b)) & 0xffu); }

// acc[j] = fma(a, q_j, acc[j]) for the sixteen codes of one lane load: one rounding per code
__device__ __forceinline__ void q8_fma16(float (&acc)[16], const uint4 &v, float a) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    acc[b] = fmaf(a, q8_code(v.x, b), acc[b]);
    acc[4 + b] = fmaf(a, q8_code(v.y, b), acc[4 + b]);
    acc[8 + b] = fmaf(a, q8_code(v.z, b), acc[8 + b]);
    acc[12 + b] = fmaf(a, q8_code(v.w, b), acc[12 + b]);
  }
}

// Decode of one code: lo + scale * q as ONE fp32 multiply and ONE fp32 add, each rounded on its own (not fused) --
// what numpy's float32 arithmetic computes, so a decoded table is the same bits on the host and on the GPU.
__device__ __forceinline__ float q8_decode(float scale, float lo, float q) { return __fadd_rn(lo, __fmul_rn(scale, q)); }

}  // namespace fgnn
