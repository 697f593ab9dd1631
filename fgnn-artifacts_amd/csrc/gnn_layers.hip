// gnn_layers.hip -- the kernels of the fused GCN and PinSAGE layers (examples/models.py: FusedGraphConv,
// FusedWeightedSAGEConv; reference: dgl.nn.GraphConv(norm='both') and the WeightedSAGEConv of
// example/samgraph/multi_gpu/train_gcn.py:24-47 / train_pinsage.py:24-75):
//   fgnn_block_degrees          both degree vectors of a block (edge counts per source, edge counts or weight sums per
//                               destination) in ONE pass over the edges -- two index_add_ passes op by op
//   fgnn_relu_l2norm (+ _backward)   ReLU + row L2 normalisation, one wave per row, one launch each way -- relu, norm,
//                               where and divide, each with a backward node of its own, op by op
// The layers' aggregation with the degree scalings inside (fgnn_block_aggregate_scaled) is the SCALED instantiation of
// the one aggregation kernel in block_aggregate.hip.
// fp32 throughout; sums are not ordered (float atomics), results agree with the torch formulation to rounding.
#include "fgnn_device.h"

namespace fgnn {
namespace {

// One lane per edge.  Sources are scattered: one float atomic per edge.  Destinations arrive seed-major, so a wave's 64
// edges fall into a few runs of equal destination: one atomic per (wave, run) -- the run's length (ballot of the run
// heads) or, weighted, the run's weight sum (segmented wave scan, added by the run's last lane).  An unsorted dst_index
// only makes the runs short.
template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void block_degrees_kernel(const uint32_t *__restrict__ src_idx,
                                                               const uint32_t *__restrict__ dst_idx,
                                                               const float *__restrict__ w, size_t num_edge,
                                                               float *src_deg, float *dst_deg) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = (uint32_t)lane_id();
  const bool live = e < num_edge;
  uint32_t my_dst = 0;
  float my_w = 0.0f;
  if (live) {
    my_dst = dst_idx[e];
    if (WEIGHTED) my_w = w[e];
    if (src_deg) unsafeAtomicAdd(&src_deg[src_idx[e]], 1.0f);
  }
  const uint32_t prev = __shfl_up(my_dst, 1, kWave);
  const bool head = live && (lane == 0 || prev != my_dst);
  const unsigned long long heads = __ballot(head);
  const uint32_t cnt = (uint32_t)__popcll(__ballot(live));  // live lanes are the wave's first cnt
  if (heads == 0ull) return;                                // wave-uniform: no edge in this wave
  if (!WEIGHTED) {
    if (head) unsafeAtomicAdd(&dst_deg[my_dst], (float)run_length_at_head(heads, lane, cnt));
  } else {
    // head of this lane's run = highest head bit at or below the lane (dead lanes: any value, they add nothing)
    const unsigned long long below = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    const uint32_t first = below ? 63u - (uint32_t)__builtin_clzll(below) : 0u;
    float s = my_w;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const float t = __shfl_up(s, d, kWave);
      if (lane >= first + (uint32_t)d) s += t;
    }
    const bool tail = live && (lane + 1 == cnt || ((heads >> (lane + 1)) & 1ull));
    if (tail) unsafeAtomicAdd(&dst_deg[my_dst], s);
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}

constexpr int kRowRegs = 4;  // a lane keeps the first 4 x 64 columns of its row in registers; wider rows are read twice

// out = relu(x) / ||relu(x)||_2 (an all-zero row stays zero: inv = 1); one wave per row, rows with the grid's stride
__global__ __launch_bounds__(kBlock) void relu_l2norm_kernel(const float *__restrict__ x, uint32_t x_ld,
                                                             float *__restrict__ out, uint32_t out_ld,
                                                             float *__restrict__ inv_norm, uint32_t rows,
                                                             uint32_t dim) {
  const uint32_t lane = (uint32_t)lane_id();
  for (uint32_t r = blockIdx.x * kWavesPerBlock + wave_id(); r < rows; r += gridDim.x * kWavesPerBlock) {
    const float *xr = x + (size_t)r * x_ld;
    float *yr = out + (size_t)r * out_ld;
    float v[kRowRegs], ss = 0.0f;
#pragma unroll
    for (int q = 0; q < kRowRegs; ++q) {
      const uint32_t c = lane + kWave * q;
      const float t = c < dim ? xr[c] : 0.0f;
      v[q] = t > 0.0f ? t : 0.0f;
      ss += v[q] * v[q];
    }
    for (uint32_t c = lane + kWave * kRowRegs; c < dim; c += kWave) {
      const float t = xr[c];
      if (t > 0.0f) ss += t * t;
    }
    ss = wave_sum(ss);
    const float inv = ss == 0.0f ? 1.0f : 1.0f / sqrtf(ss);
    if (lane == 0) inv_norm[r] = inv;
#pragma unroll
    for (int q = 0; q < kRowRegs; ++q) {
      const uint32_t c = lane + kWave * q;
      if (c < dim) yr[c] = v[q] * inv;
    }
    for (uint32_t c = lane + kWave * kRowRegs; c < dim; c += kWave) {
      const float t = xr[c];
      yr[c] = (t > 0.0f ? t : 0.0f) * inv;
    }
  }
}

// gx = (gout - out <gout, out>) * inv where out > 0, else 0.  A row whose norm was zero has out == 0 everywhere: its
// gradient is 0 (torch: the norm's gradient at 0 is 0, and relu passes nothing at x <= 0)
__global__ __launch_bounds__(kBlock) void relu_l2norm_bwd_kernel(const float *__restrict__ out, uint32_t out_ld,
                                                                 const float *__restrict__ inv_norm,
                                                                 const float *__restrict__ gout, uint32_t gout_ld,
                                                                 float *__restrict__ gx, uint32_t gx_ld, uint32_t rows,
                                                                 uint32_t dim) {
  const uint32_t lane = (uint32_t)lane_id();
  for (uint32_t r = blockIdx.x * kWavesPerBlock + wave_id(); r < rows; r += gridDim.x * kWavesPerBlock) {
    const float *yr = out + (size_t)r * out_ld;
    const float *gr = gout + (size_t)r * gout_ld;
    float *xr = gx + (size_t)r * gx_ld;
    float y[kRowRegs], g[kRowRegs], dot = 0.0f;
#pragma unroll
    for (int q = 0; q < kRowRegs; ++q) {
      const uint32_t c = lane + kWave * q;
      y[q] = c < dim ? yr[c] : 0.0f;
      g[q] = c < dim ? gr[c] : 0.0f;
      dot += g[q] * y[q];
    }
    for (uint32_t c = lane + kWave * kRowRegs; c < dim; c += kWave) dot += gr[c] * yr[c];
    dot = wave_sum(dot);
    const float inv = inv_norm[r];
#pragma unroll
    for (int q = 0; q < kRowRegs; ++q) {
      const uint32_t c = lane + kWave * q;
      if (c < dim) xr[c] = y[q] > 0.0f ? (g[q] - y[q] * dot) * inv : 0.0f;
    }
    for (uint32_t c = lane + kWave * kRowRegs; c < dim; c += kWave) {
      const float yy = yr[c];
      xr[c] = yy > 0.0f ? (gr[c] - yy * dot) * inv : 0.0f;
    }
  }
}

// rows handled by a grid of waves with a stride: enough workgroups to fill the chip, no more
inline size_t row_grid(size_t rows) {
  const size_t want = div_up(rows, (size_t)kWavesPerBlock), cap = (size_t)device_cu_count() * 8;
  return want < cap ? want : cap;
}

}  // namespace
}  // namespace fgnn

extern "C" int fgnn_block_degrees(const uint32_t *src_index, const uint32_t *dst_index, const float *edge_weight,
                                  size_t num_edge, float *src_deg, float *dst_deg, void *stream) {
  using namespace fgnn;
  if (num_edge == 0) return FGNN_OK;
  if (!dst_index || !dst_deg || (src_deg && !src_index)) return FGNN_EINVAL;
  if (!float_aligned(src_index) || !float_aligned(dst_index) || !float_aligned(edge_weight) || !float_aligned(src_deg) ||
      !float_aligned(dst_deg))
    return FGNN_EINVAL;
  const size_t blocks = div_up(num_edge, (size_t)kBlock);
  if (blocks > 0x7fffffffull) return FGNN_EINVAL;
  auto st = static_cast<hipStream_t>(stream);
  if (edge_weight)
    hipLaunchKernelGGL((block_degrees_kernel<true>), dim3(blocks), dim3(kBlock), 0, st, src_index, dst_index, edge_weight,
                       num_edge, src_deg, dst_deg);
  else
    hipLaunchKernelGGL((block_degrees_kernel<false>), dim3(blocks), dim3(kBlock), 0, st, src_index, dst_index,
                       edge_weight, num_edge, src_deg, dst_deg);
  return launch_status(__func__);
}

extern "C" int fgnn_relu_l2norm(const float *x, size_t x_ld, float *out, size_t out_ld, float *inv_norm, size_t rows,
                                size_t dim, void *stream) {
  using namespace fgnn;
  if (rows == 0) return FGNN_OK;
  if (!x || !out || !inv_norm || dim == 0 || !fits_u32(dim) || !fits_rows(rows) || x_ld < dim || !fits_u32(x_ld) ||
      out_ld < dim || !fits_u32(out_ld))
    return FGNN_EINVAL;
  if (!float_aligned(x) || !float_aligned(out) || !float_aligned(inv_norm)) return FGNN_EINVAL;
  hipLaunchKernelGGL(relu_l2norm_kernel, dim3(row_grid(rows)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), x,
                     (uint32_t)x_ld, out, (uint32_t)out_ld, inv_norm, (uint32_t)rows, (uint32_t)dim);
  return launch_status(__func__);
}

extern "C" int fgnn_relu_l2norm_backward(const float *out, size_t out_ld, const float *inv_norm, const float *gout,
                                         size_t gout_ld, float *gx, size_t gx_ld, size_t rows, size_t dim,
                                         void *stream) {
  using namespace fgnn;
  if (rows == 0) return FGNN_OK;
  if (!out || !inv_norm || !gout || !gx || dim == 0 || !fits_u32(dim) || !fits_rows(rows) || out_ld < dim ||
      !fits_u32(out_ld) || gout_ld < dim || !fits_u32(gout_ld) || gx_ld < dim || !fits_u32(gx_ld))
    return FGNN_EINVAL;
  if (!float_aligned(out) || !float_aligned(inv_norm) || !float_aligned(gout) || !float_aligned(gx)) return FGNN_EINVAL;
  hipLaunchKernelGGL(relu_l2norm_bwd_kernel, dim3(row_grid(rows)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     out, (uint32_t)out_ld, inv_norm, gout, (uint32_t)gout_ld, gx, (uint32_t)gx_ld, (uint32_t)rows,
                     (uint32_t)dim);
  return launch_status(__func__);
}
