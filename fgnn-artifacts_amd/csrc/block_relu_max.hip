// block_relu_max.hip -- GraphSAGE's max-pooling aggregator over a sampled block (dgl.nn.SAGEConv(..., 'pool');
// examples/models.py FusedSAGEPoolConv), the ReLU folded in (max(relu(.)) = relu(max(.))):
//     m[v, c]   = max over the edges e with dst_index[e] == v of x[src_index[e], c]
//     out[v, c] = m[v, c] if m[v, c] > 0 else +0.0          (a destination without an edge: +0.0)
//     arg[v, c] = the SMALLEST e with dst_index[e] == v and x[src_index[e], c] == out[v, c] if out[v, c] > 0, else -1
// Replaces relu(p)[row] (an E x D tensor), scatter_reduce_(amax) (one atomic per element) and, backward, a second E x D
// compare-and-scatter.  Where out == 0 ReLU's derivative removes the gradient, so arg = -1 is the whole backward
// information and ties at zero need no rule.  Inputs are finite: what a NaN does is unspecified (it never wins a
// comparison here, torch's amax would propagate it).
// Forward, three launches on one stream, every x row read once, nothing of size E x D written:
//   1. zero the key table ws[num_dst x dim] of 64-bit words: "no positive value yet" = "out 0, arg -1"
//   2. block_relu_max_kernel, block_aggregate_kernel's work split: a wave owns kEdgesPerWave consecutive edges and
//      broadcasts their indices by shuffle, lane l owns columns l + 64 q, four row loads are in flight.  While the
//      destination does not change the running (value, edge) pair of every owned column stays in registers (a strict >
//      over ascending e keeps the smallest tied edge); only a run boundary touches memory.  Positive floats order like
//      their bit patterns, so ONE 64-bit atomic max of (float bits << 32) | (0xFFFFFFFF - e) per (wave, run, column)
//      yields the maximum and the smallest tied edge at once, whatever the order of the edges and however a
//      destination's edges are spread over waves.  A column whose running maximum is <= 0 issues no atomic.
//   3. unpack the table into out (OVERWRITTEN; may be a column block of a wider matrix) and arg.
// Backward: waves own destination rows, lanes columns; arg and gout are read coalesced, src_index[arg] is gathered and
// one hardware float atomic per live element adds into the caller-initialised gx.  An element of gx receives at most
// one term per (destination, column) that selected it: the (k + 8) 2^-23 bound of block_aggregate.hip holds.
#include "aggregate_rows.h"

namespace fgnn {
namespace {

using Key = unsigned long long;

__global__ __launch_bounds__(kBlock) void relu_max_zero_kernel(Key *keys, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) keys[i] = 0ull;
}

// P slots of one column per lane and pass over the edges (dim <= 64 P: one pass).  All lanes run the edge loop (the
// shuffles need them); loads and atomics are masked by column < dim.
template <int P>
__global__ __launch_bounds__(kBlock) void block_relu_max_kernel(const uint32_t *__restrict__ src_idx,
                                                                const uint32_t *__restrict__ dst_idx,
                                                                const float *__restrict__ x, Key *keys, size_t num_edge,
                                                                uint32_t num_dst, uint32_t dim, uint32_t x_ld) {
  const size_t wave = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  const size_t e0 = wave * kEdgesPerWave;
  if (e0 >= num_edge) return;  // wave-uniform
  const size_t e1 = e0 + kEdgesPerWave < num_edge ? e0 + kEdgesPerWave : num_edge;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t cnt = (uint32_t)(e1 - e0);
  uint32_t my_src = 0, my_dst = 0;  // lane i holds edge e0 + i
  if (lane < cnt) {
    my_src = src_idx[e0 + lane];
    my_dst = dst_idx[e0 + lane];
  }
  for (uint32_t dbase = 0; dbase < dim; dbase += kWave * P) {
    bool act[P];
    float best[P];       // running maximum of the run, 0 = nothing positive yet
    uint32_t best_e[P];  // its edge (low word of e: num_edge < 2^31)
#pragma unroll
    for (int q = 0; q < P; ++q) {
      act[q] = dbase + lane + kWave * q < dim;
      best[q] = 0.0f;
      best_e[q] = 0u;
    }
    uint32_t cur = __shfl(my_dst, 0, kWave);
    // the run boundary (wave-uniform): one 64-bit atomic max per column that saw a positive value; a destination
    // outside the table (a violated contract) is dropped rather than written out of bounds
    auto flush = [&](uint32_t dst) {
      Key *kp = keys + (size_t)dst * dim + dbase + lane;
#pragma unroll
      for (int q = 0; q < P; ++q) {
        if (act[q] && best[q] > 0.0f && dst < num_dst)
          atomicMax(kp + kWave * q, ((Key)__float_as_uint(best[q]) << 32) | (Key)(0xFFFFFFFFu - best_e[q]));
        best[q] = 0.0f;
      }
    };
    constexpr uint32_t UN = 4;  // edges whose row loads are in flight together
    for (uint32_t i0 = 0; i0 < cnt; i0 += UN) {
      float v[UN][P];
      uint32_t c[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t i = i0 + u < cnt ? i0 + u : cnt - 1;  // clamp: the extra loads are discarded below
        const uint32_t sidx = __shfl(my_src, (int)i, kWave);
        c[u] = __shfl(my_dst, (int)i, kWave);
        const float *xp = x + (size_t)sidx * x_ld + dbase + lane;
#pragma unroll
        for (int q = 0; q < P; ++q) v[u][q] = act[q] ? xp[kWave * q] : 0.0f;
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (i0 + u >= cnt) break;  // wave-uniform
        if (c[u] != cur) {         // wave-uniform: run boundary
          flush(cur);
          cur = c[u];
        }
        const uint32_t e = (uint32_t)e0 + i0 + u;
#pragma unroll
        for (int q = 0; q < P; ++q) {
          if (v[u][q] > best[q]) {  // strict: of equal values the earlier edge stays
            best[q] = v[u][q];
            best_e[q] = e;
          }
        }
      }
    }
    flush(cur);
  }
}

// key table -> out (row stride out_ld) and arg [num_dst, dim]; thread i takes element i of the table
__global__ __launch_bounds__(kBlock) void relu_max_unpack_kernel(const Key *__restrict__ keys, float *out, int32_t *arg,
                                                                 size_t n, uint32_t dim, uint32_t out_ld) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const Key k = keys[i];
    const size_t v = i / dim;
    const uint32_t c = (uint32_t)(i - v * dim);
    out[v * out_ld + c] = __uint_as_float((uint32_t)(k >> 32));  // no key: bits 0 = +0.0
    arg[i] = k ? (int32_t)(0xFFFFFFFFu - (uint32_t)k) : -1;
  }
}

// A wave per destination row (grid-stride), lane l columns l + 64 j, UN of them per trip so that the arg loads, the
// src_index gathers and the gout loads of a trip overlap.  An arg outside [0, num_edge) adds nothing.
__global__ __launch_bounds__(kBlock) void block_relu_max_bwd_kernel(const int32_t *__restrict__ arg,
                                                                    const uint32_t *__restrict__ src_idx,
                                                                    uint32_t num_edge, const float *__restrict__ gout,
                                                                    uint32_t gout_ld, uint32_t num_dst, uint32_t dim,
                                                                    float *gx, uint32_t gx_ld) {
  constexpr uint32_t UN = 4;
  const uint32_t lane = (uint32_t)lane_id();
  for (uint32_t r = blockIdx.x * kWavesPerBlock + wave_id(); r < num_dst; r += gridDim.x * kWavesPerBlock) {
    const int32_t *ar = arg + (size_t)r * dim;
    const float *gr = gout + (size_t)r * gout_ld;
    for (uint32_t c0 = lane; c0 < dim; c0 += kWave * UN) {
      int32_t a[UN];
      uint32_t s[UN];
      float g[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t c = c0 + kWave * u;
        a[u] = c < dim ? ar[c] : -1;
        if ((uint32_t)a[u] >= num_edge) a[u] = -1;  // (negative values are >= 2^31 as unsigned)
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        s[u] = a[u] >= 0 ? src_idx[a[u]] : 0u;
        g[u] = a[u] >= 0 ? gr[c0 + kWave * u] : 0.0f;
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u)
        if (a[u] >= 0) unsafeAtomicAdd(gx + (size_t)s[u] * gx_ld + c0 + kWave * u, g[u]);
    }
  }
}

// grid of an elementwise pass over n items: a few workgroups per CU at most, the kernels stride
inline size_t flat_grid(size_t n) {
  const size_t want = div_up(n, (size_t)kBlock), cap = (size_t)device_cu_count() * 8;
  return want < cap ? want : cap;
}

}  // namespace
}  // namespace fgnn

extern "C" size_t fgnn_block_relu_max_workspace_bytes(size_t num_dst, size_t dim) {
  return num_dst * dim * sizeof(fgnn::Key);
}

extern "C" int fgnn_block_relu_max_forward(const uint32_t *src_index, const uint32_t *dst_index, size_t num_edge,
                                           const float *x, size_t x_ld, size_t num_dst, size_t dim, float *out,
                                           size_t out_ld, int32_t *arg, void *ws, size_t ws_bytes, void *stream) {
  using namespace fgnn;
  if (num_dst == 0) return FGNN_OK;
  if (num_edge > 0x7fffffffull) return FGNN_EINVAL;  // arg is int32
  if (!out || !arg || !ws || dim == 0 || !fits_u32(dim) || !fits_rows(num_dst) || out_ld < dim || !fits_u32(out_ld) ||
      !float_aligned(out) || !float_aligned(arg) || (reinterpret_cast<uintptr_t>(ws) & 7u) != 0)
    return FGNN_EINVAL;
  if (num_edge && (!src_index || !dst_index || !x || x_ld < dim || !fits_u32(x_ld) || !float_aligned(src_index) ||
                   !float_aligned(dst_index) || !float_aligned(x)))
    return FGNN_EINVAL;
  if (num_dst > ((size_t)-1) / sizeof(Key) / dim || ws_bytes < num_dst * dim * sizeof(Key)) return FGNN_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  Key *keys = static_cast<Key *>(ws);
  const size_t n = num_dst * dim;
  hipLaunchKernelGGL(relu_max_zero_kernel, dim3(flat_grid(n)), dim3(kBlock), 0, s, keys, n);
  if (num_edge) {
    const size_t blocks = div_up(div_up(num_edge, (size_t)kEdgesPerWave), (size_t)kWavesPerBlock);
    auto kernel = dim <= (size_t)kWave ? block_relu_max_kernel<1>
                                       : (dim <= 2 * (size_t)kWave ? block_relu_max_kernel<2> : block_relu_max_kernel<4>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, s, src_index, dst_index, x, keys, num_edge,
                       (uint32_t)num_dst, (uint32_t)dim, (uint32_t)x_ld);
  }
  hipLaunchKernelGGL(relu_max_unpack_kernel, dim3(flat_grid(n)), dim3(kBlock), 0, s, keys, out, arg, n, (uint32_t)dim,
                     (uint32_t)out_ld);
  return launch_status(__func__);
}

extern "C" int fgnn_block_relu_max_backward(const int32_t *arg, const uint32_t *src_index, size_t num_edge,
                                            const float *gout, size_t gout_ld, size_t num_dst, size_t dim, float *gx,
                                            size_t gx_ld, void *stream) {
  using namespace fgnn;
  if (num_dst == 0 || num_edge == 0) return FGNN_OK;  // no edge: every arg is -1
  if (num_edge > 0x7fffffffull) return FGNN_EINVAL;
  if (!arg || !src_index || !gout || !gx || dim == 0 || !fits_u32(dim) || !fits_rows(num_dst) || gout_ld < dim ||
      !fits_u32(gout_ld) || gx_ld < dim || !fits_u32(gx_ld) || !float_aligned(arg) || !float_aligned(src_index) ||
      !float_aligned(gout) || !float_aligned(gx))
    return FGNN_EINVAL;
  const size_t want = div_up(num_dst, (size_t)kWavesPerBlock), cap = (size_t)device_cu_count() * 8;
  hipLaunchKernelGGL(block_relu_max_bwd_kernel, dim3(want < cap ? want : cap), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), arg, src_index, (uint32_t)num_edge, gout, (uint32_t)gout_ld,
                     (uint32_t)num_dst, (uint32_t)dim, gx, (uint32_t)gx_ld);
  return launch_status(__func__);
}
