// block_aggregate.hip -- neighbourhood aggregation over a sampled block (the message-passing step of the DGL-free
// SAGEConv / GraphConv / PinSAGE layers in examples/models.py):
//     out[col[e], :] += w[e] * h[row[e], :]        for every edge e of the block
// Replaces torch's `h[row]` (materialises an E x D tensor) + `index_add_` (one float atomic per element): rows are
// read once straight from h, products are accumulated in registers while consecutive edges share their destination
// (the samplers emit edges seed-major, so a destination's edges are contiguous) and only segment boundaries touch
// memory, with hardware float atomics (a segment may continue in the next wave's chunk).  The same kernel with row
// and col swapped is the backward pass (grad_h[row[e]] += w[e] * grad_out[col[e]]).  Sums in fp32; the order of the
// additions is not fixed; against a float64 reference every output stays within (k + 8) 2^-23 of the sum of its terms'
// magnitudes, k = the destination's edge count (tests/test_train_kernel_references_gpu.py; observed: 0.15 of that).
// ONE kernel template serves all entry points.  fgnn_block_aggregate / fgnn_block_aggregate_ex: the plain sum,
// with the destinations' in-degrees counted on the way if asked for.  fgnn_block_aggregate_scaled (SCALED
// instantiations; the fused GCN and PinSAGE layers): the layers' degree scalings ride along -- the per-source factor is
// folded into the broadcast edge weight, the per-destination factor multiplies every flushed partial sum.  Both are
// linear, so no scaled copy of h (num_src x D, the largest tensor of a step) is ever written, and the backward pass is
// the same launch with indices, degree vectors and modes swapped.
// fgnn_block_aggregate_ex_f16 / _scaled_f16 (the first layer over a half-precision feature store): the rows of h are
// IEEE binary16, converted on load (exact); weights, sums and out stay fp32, so an output element sees the very
// additions, in the very order, that the fp32 entry points make on the upcast rows.
#include "aggregate_rows.h"

namespace fgnn {
namespace {

// Lane l owns slots l, l + 64, ... (P of them per pass over the edges), a slot being kRowCols<Row> adjacent columns:
// every load of a wave instruction covers 64 consecutive slots (256 bytes of a row for float and __half2), every float
// atomic 64 consecutive columns (see the flush for two-column slots).  All lanes run the edge loop (the
// shuffles need them), memory operations are masked by the slot's first column < dim (two-column slots are only used
// with even dim).  SCALED: lane i's weight is multiplied by its source's degree factor and the destination factor of
// its segment travels beside it; the other instantiations carry neither.
template <int P, bool SCALED, typename Row>
__global__ __launch_bounds__(kBlock) void block_aggregate_kernel(
    const uint32_t *__restrict__ src_idx, const uint32_t *__restrict__ dst_idx, const float *__restrict__ w,
    const Row *__restrict__ h, float *out, size_t num_edge, uint32_t dim, uint32_t h_ld, uint32_t out_ld, float *deg,
    const float *__restrict__ src_deg, int src_mode, const float *__restrict__ dst_deg, int dst_mode) {
  constexpr int V = kRowCols<Row>;
  const size_t wave = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  const size_t e0 = wave * kEdgesPerWave;
  if (e0 >= num_edge) return;  // wave-uniform
  const size_t e1 = e0 + kEdgesPerWave < num_edge ? e0 + kEdgesPerWave : num_edge;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t cnt = (uint32_t)(e1 - e0);
  // the chunk's edges: lane i holds edge e0 + i; the loop below broadcasts them with wave shuffles instead of
  // issuing a dependent (index -> row) load chain per edge
  uint32_t my_src = 0, my_dst = 0;
  float my_w = 1.0f;
  [[maybe_unused]] float my_fd = 1.0f;
  if (lane < cnt) {
    my_src = src_idx[e0 + lane];
    my_dst = dst_idx[e0 + lane];
    if (w) my_w = w[e0 + lane];
    if constexpr (SCALED) {
      if (src_mode) my_w *= degree_factor(src_deg[my_src], src_mode);
      if (dst_mode) my_fd = degree_factor(dst_deg[my_dst], dst_mode);
    }
  }
  // in-degrees on the way (deg != null): the first lane of every run of equal destinations adds the run's length --
  // one float atomic per (wave, destination) instead of an index_add_ pass of its own over the edges
  if (deg) {
    const uint32_t prev = __shfl_up(my_dst, 1, kWave);
    const bool head = lane < cnt && (lane == 0 || prev != my_dst);
    const unsigned long long heads = __ballot(head);
    if (head) unsafeAtomicAdd(&deg[my_dst], (float)run_length_at_head(heads, lane, cnt));
  }
  for (uint32_t dbase = 0; dbase < dim; dbase += kWave * P * V) {  // one trip for dim <= 64 P V
    bool act[P];
    float acc[P][V];
#pragma unroll
    for (int q = 0; q < P; ++q) {
      act[q] = dbase + (lane + kWave * q) * V < dim;
#pragma unroll
      for (int j = 0; j < V; ++j) acc[q][j] = 0.0f;
    }
    uint32_t cur = __shfl(my_dst, 0, kWave);
    [[maybe_unused]] float cur_fd = 1.0f;
    if constexpr (SCALED) cur_fd = __shfl(my_fd, 0, kWave);
    // what a flush adds for the partial sum a: the destination factor is applied here, once per segment
    auto flushed = [&](float a) {
      if constexpr (SCALED) return cur_fd * a;
      else return a;
    };
    // the flush itself (wave-uniform).  One column per slot: lane l adds column dbase + l + 64 q.  Two columns per
    // slot: the lane's pair (2 l, 2 l + 1) of the slot's 128 columns would make every atomic instruction touch every
    // other float of 512 bytes -- twice the lines per instruction, and blocks with a handful of edges per destination
    // are bound by exactly that -- so the sums change lanes first: instruction j of a slot covers its columns
    // 64 j .. 64 j + 63, lane l taking column 64 j + l from lane 32 j + l / 2.  The values are moved, not changed.
    auto flush = [&](uint32_t dst) {
      float *op = out + (size_t)dst * out_ld + dbase + lane;
#pragma unroll
      for (int q = 0; q < P; ++q) {
        if constexpr (V == 1) {
          if (act[q]) unsafeAtomicAdd(op + kWave * q, flushed(acc[q][0]));
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const int from = 32 * j + (int)(lane >> 1);
            const float lo = __shfl(acc[q][0], from, kWave), hi = __shfl(acc[q][V - 1], from, kWave);
            if (dbase + kWave * (V * q + j) + lane < dim)
              unsafeAtomicAdd(op + kWave * (V * q + j), flushed((lane & 1u) ? hi : lo));
          }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) acc[q][j] = 0.0f;
      }
    };
    constexpr uint32_t UN = 4;  // edges whose row loads are in flight together
    for (uint32_t i0 = 0; i0 < cnt; i0 += UN) {
      Row v[UN][P];
      uint32_t c[UN];
      float we[UN];
      [[maybe_unused]] float fd[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t i = i0 + u < cnt ? i0 + u : cnt - 1;  // clamp: the extra loads are discarded below
        const uint32_t sidx = __shfl(my_src, (int)i, kWave);
        c[u] = __shfl(my_dst, (int)i, kWave);
        we[u] = __shfl(my_w, (int)i, kWave);
        if constexpr (SCALED) fd[u] = __shfl(my_fd, (int)i, kWave);
        // (h_ld and dbase are multiples of V wherever V == 2)
        const Row *hp = h + ((size_t)sidx * h_ld + dbase) / V + lane;
#pragma unroll
        for (int q = 0; q < P; ++q) v[u][q] = act[q] ? hp[kWave * q] : row_zero<Row>();
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (i0 + u >= cnt) break;  // wave-uniform
        if (c[u] != cur) {         // wave-uniform: segment boundary, flush
          flush(cur);
          cur = c[u];
          if constexpr (SCALED) cur_fd = fd[u];
        }
#pragma unroll
        for (int q = 0; q < P; ++q) {
#pragma unroll
          for (int j = 0; j < V; ++j) acc[q][j] += we[u] * row_col(v[u][q], j);
        }
      }
    }
    flush(cur);
  }
}

// the launch for one row type: the choice of instantiation (slots per lane by dim; SCALED by entry point -- the scaled
// one keeps its instantiation for modes 0 / 0 too)
template <typename Row, typename... Args>
void launch_rows(bool scaled, size_t dim, size_t blocks, hipStream_t stream, const void *h, const uint32_t *src_index,
                 const uint32_t *dst_index, const float *edge_weight, Args... rest) {
  using Kernel = decltype(&block_aggregate_kernel<1, false, Row>);
  static constexpr Kernel kernels[2][3] = {
      {block_aggregate_kernel<1, false, Row>, block_aggregate_kernel<2, false, Row>,
       block_aggregate_kernel<4, false, Row>},
      {block_aggregate_kernel<1, true, Row>, block_aggregate_kernel<2, true, Row>, block_aggregate_kernel<4, true, Row>}};
  constexpr size_t pass = (size_t)kWave * kRowCols<Row>;  // columns of a pass at one slot per lane
  hipLaunchKernelGGL(kernels[scaled][dim <= pass ? 0 : (dim <= 2 * pass ? 1 : 2)], dim3(blocks), dim3(kBlock), 0, stream,
                     src_index, dst_index, edge_weight, static_cast<const Row *>(h), rest...);
}

// The one way to a launch: argument checks, grid, and the row type (h_f16: h holds binary16 rows, 2-byte aligned; they
// are read two columns per lane unless the base, the stride or dim is odd).
int launch_block_aggregate(const char *what, bool scaled, bool h_f16, const uint32_t *src_index,
                           const uint32_t *dst_index, const float *edge_weight, size_t num_edge, const void *h,
                           size_t h_ld, size_t dim, float *out, size_t out_ld, float *in_degree, const float *src_deg,
                           int src_mode, const float *dst_deg, int dst_mode, void *stream) {
  if (num_edge == 0) return FGNN_OK;
  if (!src_index || !dst_index || !float_aligned(src_index) || !float_aligned(dst_index) || !float_aligned(in_degree) ||
      !aggregate_args_ok(h_f16, h, h_ld, dim, out, out_ld, edge_weight, src_deg, src_mode, dst_deg, dst_mode))
    return FGNN_EINVAL;
  const size_t waves = div_up(num_edge, (size_t)kEdgesPerWave);
  const size_t blocks = div_up(waves, (size_t)kWavesPerBlock);
  if (blocks > 0x7fffffffull) return FGNN_EINVAL;
  auto launch = [&](auto row) {
    launch_rows<decltype(row)>(scaled, dim, blocks, static_cast<hipStream_t>(stream), h, src_index, dst_index,
                               edge_weight, out, num_edge, (uint32_t)dim, (uint32_t)h_ld, (uint32_t)out_ld, in_degree,
                               src_deg, src_mode, dst_deg, dst_mode);
  };
  if (!h_f16) launch(float());
  else if (half_rows_paired(h, h_ld, dim)) launch(__half2());
  else launch(__half());
  return launch_status(what);
}

}  // namespace
}  // namespace fgnn

extern "C" int fgnn_block_aggregate_ex(const uint32_t *src_index, const uint32_t *dst_index, const float *edge_weight,
                                       size_t num_edge, const float *h, size_t dim, float *out, size_t out_ld,
                                       float *in_degree, void *stream) {
  return fgnn::launch_block_aggregate(__func__, false, false, src_index, dst_index, edge_weight, num_edge, h, dim, dim,
                                      out, out_ld, in_degree, nullptr, 0, nullptr, 0, stream);
}

extern "C" int fgnn_block_aggregate(const uint32_t *src_index, const uint32_t *dst_index, const float *edge_weight,
                                    size_t num_edge, const float *h, size_t dim, float *out, void *stream) {
  return fgnn::launch_block_aggregate(__func__, false, false, src_index, dst_index, edge_weight, num_edge, h, dim, dim,
                                      out, dim, nullptr, nullptr, 0, nullptr, 0, stream);
}

extern "C" int fgnn_block_aggregate_scaled(const uint32_t *src_index, const uint32_t *dst_index,
                                           const float *edge_weight, size_t num_edge, const float *h, size_t h_ld,
                                           size_t dim, float *out, size_t out_ld, const float *src_deg, int src_mode,
                                           const float *dst_deg, int dst_mode, void *stream) {
  return fgnn::launch_block_aggregate(__func__, true, false, src_index, dst_index, edge_weight, num_edge, h, h_ld, dim,
                                      out, out_ld, nullptr, src_deg, src_mode, dst_deg, dst_mode, stream);
}

extern "C" int fgnn_block_aggregate_ex_f16(const uint32_t *src_index, const uint32_t *dst_index,
                                           const float *edge_weight, size_t num_edge, const void *h, size_t dim,
                                           float *out, size_t out_ld, float *in_degree, void *stream) {
  return fgnn::launch_block_aggregate(__func__, false, true, src_index, dst_index, edge_weight, num_edge, h, dim, dim,
                                      out, out_ld, in_degree, nullptr, 0, nullptr, 0, stream);
}

extern "C" int fgnn_block_aggregate_scaled_f16(const uint32_t *src_index, const uint32_t *dst_index,
                                               const float *edge_weight, size_t num_edge, const void *h, size_t h_ld,
                                               size_t dim, float *out, size_t out_ld, const float *src_deg,
                                               int src_mode, const float *dst_deg, int dst_mode, void *stream) {
  return fgnn::launch_block_aggregate(__func__, true, true, src_index, dst_index, edge_weight, num_edge, h, h_ld, dim,
                                      out, out_ld, nullptr, src_deg, src_mode, dst_deg, dst_mode, stream);
}
