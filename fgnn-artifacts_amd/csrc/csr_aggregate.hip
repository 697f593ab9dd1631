// csr_aggregate.hip -- neighbourhood aggregation over whole CSR rows: the message-passing step of exact layer-wise
// inference on the full graph (examples/inference.py).  For output row i, v = nodes ? nodes[i] : first + i:
//     out[i, c] = f_dst(v) * sum over p in [indptr[v], indptr[v + 1]) of  w[p] * f_src(indices[p]) * h[indices[p], c]
// block_aggregate.hip serves sampled COO blocks: an explicit destination per edge, float atomics into a zero-filled
// output, no fixed order of the additions.  A CSR row needs none of that: its edges are one contiguous run, so ONE wave
// owns the output row, sums it in registers and stores it once -- out is overwritten (no zero fill: it is usually the
// right half of a SAGE z), a row without a neighbour writes zeros, there is no atomic on a float anywhere.
// The order of the additions is fixed by the row alone.  A row is cut into pieces of kCsrSplit edges (the last one
// shorter); a piece's sum starts at 0 and adds its edges' products in CSR order; the row's sum starts at 0 and adds the
// piece sums in piece order; the destination factor multiplies that once.  Who computes a piece does not enter: rows of
// at most kCsrSplit edges (one piece) and rows the workspace has no room for are summed by their owner wave, longer
// rows -- the hubs of a power-law graph, 10^5 .. 10^6 neighbours, tens of milliseconds for one wave -- are appended to a
// queue in the workspace by the row pass (csr_queue.h; device-side counters; the queue order varies), their pieces
// summed into partial rows of the workspace by the waves of a second launch and combined in piece order by a third.
// So a node's result is bit for bit the same in a call over [0, N) and in a call over 7 nodes, today and tomorrow.
// Three stream-ordered launches (one where no row of the call can be a hub), one 16-byte memset, no host
// synchronisation, no copy to the host.  Sums in fp32; h is fp32 or binary16 upcast on load (exact).  Against a float64
// reference every output stays within (k + 8) 2^-23 of the sum of its terms' magnitudes, k = the row's length
// (tests/test_csr_aggregate_gpu.py), the bound block_aggregate.hip documents.
// Index widths: edge positions are uint32_t (E < 2^32 is the dataset contract); every address into h, out and the
// partial rows is formed in size_t (111 M rows x 256 columns overflow 32 bits).
#include "aggregate_rows.h"
#include "csr_queue.h"

namespace fgnn {
namespace {

// The graph, the rows asked for and the scalings: what all three kernels read.
struct CsrJob {
  const uint32_t *indptr, *indices, *nodes;
  const float *w, *src_deg, *dst_deg;
  uint32_t first;
  int src_mode, dst_mode;
};
__device__ __forceinline__ uint32_t job_node(const CsrJob &j, size_t i) { return j.nodes ? j.nodes[i] : j.first + (uint32_t)i; }
// dst_deg == null: the row's own length is the degree (SAGE's mean, GCN's in-degree norm on the full graph)
__device__ __forceinline__ float job_dst_factor(const CsrJob &j, uint32_t v, uint32_t len) {
  return j.dst_mode ? degree_factor(j.dst_deg ? j.dst_deg[v] : (float)len, j.dst_mode) : 1.0f;
}

// Lane l owns slots l, l + 64, ... (P per pass over the edges), a slot being kRowCols<Row> adjacent columns, as in
// block_aggregate_kernel.  acc[q][j] += the products of the cnt (<= kCsrSplit) edges from position p0 on, in CSR order,
// for the columns of pass dbase.  The wave's lanes load 64 neighbour ids (and weights) at a time, coalesced, and
// broadcast them by shuffle; UN row loads are in flight together.  All lanes run the loop (the shuffles need them),
// loads are masked by act[q].
template <int P, typename Row>
__device__ __forceinline__ void sum_piece(float (&acc)[P][kRowCols<Row>], const bool (&act)[P], const CsrJob &job,
                                          const Row *__restrict__ h, uint32_t h_ld, uint32_t dbase, uint32_t p0,
                                          uint32_t cnt, uint32_t lane) {
  constexpr int V = kRowCols<Row>;
  constexpr uint32_t UN = 4;
  for (uint32_t c0 = 0; c0 < cnt; c0 += kWave) {
    const uint32_t n = cnt - c0 < (uint32_t)kWave ? cnt - c0 : (uint32_t)kWave;
    uint32_t my_src = 0;
    float my_w = 1.0f;
    if (lane < n) {
      const uint32_t p = p0 + c0 + lane;
      my_src = job.indices[p];
      if (job.w) my_w = job.w[p];
      if (job.src_mode) my_w *= degree_factor(job.src_deg[my_src], job.src_mode);
    }
    for (uint32_t i0 = 0; i0 < n; i0 += UN) {
      Row v[UN][P];
      float we[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t i = i0 + u < n ? i0 + u : n - 1;  // clamp: the extra loads are discarded below
        const uint32_t sidx = __shfl(my_src, (int)i, kWave);
        we[u] = __shfl(my_w, (int)i, kWave);
        // (h_ld and dbase are multiples of V wherever V == 2)
        const Row *hp = h + ((size_t)sidx * h_ld + dbase) / V + lane;
#pragma unroll
        for (int q = 0; q < P; ++q) v[u][q] = act[q] ? hp[kWave * q] : row_zero<Row>();
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (i0 + u >= n) break;  // wave-uniform
#pragma unroll
        for (int q = 0; q < P; ++q) {
#pragma unroll
          for (int j = 0; j < V; ++j) acc[q][j] += we[u] * row_col(v[u][q], j);
        }
      }
    }
  }
}

// Stores val[q][j] * scale to the columns of pass dbase of the row at `op` (plain vector stores, 64 consecutive columns
// per instruction).  Two-column slots change lanes first, as in block_aggregate_kernel's flush: instruction j of a slot
// covers its columns 64 j .. 64 j + 63, lane l taking column 64 j + l from lane 32 j + l / 2.
template <int P, int V>
__device__ __forceinline__ void store_pass(float *op, const float (&val)[P][V], float scale, uint32_t dbase, uint32_t dim,
                                           uint32_t lane) {
#pragma unroll
  for (int q = 0; q < P; ++q) {
    if constexpr (V == 1) {
      const uint32_t c = dbase + kWave * q + lane;
      if (c < dim) op[c] = scale * val[q][0];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int from = 32 * j + (int)(lane >> 1);
        const float lo = __shfl(val[q][0], from, kWave), hi = __shfl(val[q][V - 1], from, kWave);
        const uint32_t c = dbase + kWave * (V * q + j) + lane;
        if (c < dim) op[c] = scale * ((lane & 1u) ? hi : lo);
      }
    }
  }
}

template <int P, typename Row>
__device__ __forceinline__ void set_active(bool (&act)[P], uint32_t dbase, uint32_t dim, uint32_t lane) {
#pragma unroll
  for (int q = 0; q < P; ++q) act[q] = dbase + (lane + kWave * q) * kRowCols<Row> < dim;
}

// Row pass: wave (blockIdx.x, wave_id) owns output row i.  A row of more than kCsrSplit edges goes to the hub queue if
// the workspace has room for it (it always has when the caller's max_edges holds); otherwise its owner sums it here,
// piece by piece -- the same additions in the same order.
template <int P, typename Row>
__global__ __launch_bounds__(kBlock) void csr_rows_kernel(CsrJob job, CsrWs ws, const Row *__restrict__ h, float *out,
                                                          size_t num_rows, uint32_t dim, uint32_t h_ld,
                                                          uint32_t out_ld) {
  constexpr int V = kRowCols<Row>;
  const size_t i = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  if (i >= num_rows) return;  // wave-uniform
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t v = job_node(job, i);
  const uint32_t beg = job.indptr[v], len = job.indptr[v + 1] - beg;
  const uint32_t np = piece_count(len);
  if (np > 1 && ws.hub_cap && csr_queue_hub(ws, (uint32_t)i, np, lane)) return;  // wave-uniform
  const float fd = job_dst_factor(job, v, len);
  float *op = out + i * out_ld;
  for (uint32_t dbase = 0; dbase < dim; dbase += kWave * P * V) {  // one trip for dim <= 64 P V
    bool act[P];
    set_active<P, Row>(act, dbase, dim, lane);
    float total[P][V] = {};
    for (uint32_t k = 0; k < np; ++k) {
      float acc[P][V] = {};
      const uint32_t done = k * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
      sum_piece<P, Row>(acc, act, job, h, h_ld, dbase, beg + done, cnt, lane);
#pragma unroll
      for (int q = 0; q < P; ++q) {
#pragma unroll
        for (int j = 0; j < V; ++j) total[q][j] += acc[q][j];
      }
    }
    store_pass<P, V>(op, total, fd, dbase, dim, lane);
  }
}

// Hub pass 1: the waves of the grid walk the piece descriptors the row pass wrote (their number is read from device
// memory) and leave every piece's sum in its partial row.
template <int P, typename Row>
__global__ __launch_bounds__(kBlock) void csr_hub_pieces_kernel(CsrJob job, CsrWs ws, const Row *__restrict__ h,
                                                                uint32_t dim, uint32_t h_ld) {
  constexpr int V = kRowCols<Row>;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t handed = ws.counts[1], n = handed < ws.piece_cap ? handed : ws.piece_cap;
  const uint32_t stride = gridDim.x * kWavesPerBlock;
  for (uint32_t p = blockIdx.x * kWavesPerBlock + wave_id(); p < n; p += stride) {
    const uint2 d = ws.pieces[p];
    if (d.x == kNoRow) continue;  // wave-uniform
    const uint32_t v = job_node(job, d.x);
    const uint32_t beg = job.indptr[v], len = job.indptr[v + 1] - beg;
    const uint32_t done = d.y * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
    float *pp = ws.partial + (size_t)p * dim;
    for (uint32_t dbase = 0; dbase < dim; dbase += kWave * P * V) {
      bool act[P];
      set_active<P, Row>(act, dbase, dim, lane);
      float acc[P][V] = {};
      sum_piece<P, Row>(acc, act, job, h, h_ld, dbase, beg + done, cnt, lane);
      store_pass<P, V>(pp, acc, 1.0f, dbase, dim, lane);
    }
  }
}

// Hub pass 2: one wave per (queued hub, 64 columns) adds the hub's partial rows IN PIECE ORDER, starting at 0 -- the
// additions the row pass makes for a row it sums itself -- and stores the output row.  UN partial loads are in flight
// together; the additions stay sequential.
__global__ __launch_bounds__(kBlock) void csr_hub_combine_kernel(CsrJob job, CsrWs ws, float *out, uint32_t dim,
                                                                 uint32_t out_ld) {
  constexpr uint32_t UN = 8;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t queued = ws.counts[0], nh = queued < ws.hub_cap ? queued : ws.hub_cap;
  const uint32_t chunks = (dim + kWave - 1) / kWave;
  const size_t items = (size_t)nh * chunks, stride = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t it = (size_t)blockIdx.x * kWavesPerBlock + wave_id(); it < items; it += stride) {
    const uint2 hub = ws.hubs[it / chunks];
    if (hub.x == kNoRow) continue;  // wave-uniform
    const uint32_t c = (uint32_t)(it % chunks) * kWave + lane;
    const uint32_t v = job_node(job, hub.x);
    const uint32_t len = job.indptr[v + 1] - job.indptr[v], np = piece_count(len);
    const float *pp = ws.partial + (size_t)hub.y * dim + c;
    float total = 0.0f;
    for (uint32_t k0 = 0; k0 < np; k0 += UN) {
      float t[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) t[u] = (c < dim && k0 + u < np) ? pp[(size_t)(k0 + u) * dim] : 0.0f;
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (k0 + u >= np) break;  // wave-uniform
        total += t[u];
      }
    }
    if (c < dim) out[(size_t)hub.x * out_ld + c] = job_dst_factor(job, v, len) * total;
  }
}

// the launches for one row type: the instantiation by dim (slots per lane), the hub passes where a hub is possible
template <typename Row>
void launch_csr(const CsrJob &job, const CsrWs &ws, const void *h, float *out, size_t num_rows, uint32_t dim,
                uint32_t h_ld, uint32_t out_ld, hipStream_t stream) {
  static constexpr decltype(&csr_rows_kernel<1, Row>) rows[3] = {csr_rows_kernel<1, Row>, csr_rows_kernel<2, Row>,
                                                                 csr_rows_kernel<4, Row>};
  static constexpr decltype(&csr_hub_pieces_kernel<1, Row>) pieces[3] = {
      csr_hub_pieces_kernel<1, Row>, csr_hub_pieces_kernel<2, Row>, csr_hub_pieces_kernel<4, Row>};
  constexpr size_t pass = (size_t)kWave * kRowCols<Row>;  // columns of a pass at one slot per lane
  const int which = dim <= pass ? 0 : (dim <= 2 * pass ? 1 : 2);
  const Row *hr = static_cast<const Row *>(h);
  hipLaunchKernelGGL(rows[which], dim3(div_up(num_rows, (size_t)kWavesPerBlock)), dim3(kBlock), 0, stream, job, ws, hr,
                     out, num_rows, dim, h_ld, out_ld);
  if (!ws.hub_cap) return;
  const size_t pg = div_up((size_t)ws.piece_cap, (size_t)kWavesPerBlock);
  hipLaunchKernelGGL(pieces[which], dim3(pg < kHubGridBlocks ? pg : kHubGridBlocks), dim3(kBlock), 0, stream, job, ws,
                     hr, dim, h_ld);
  const size_t cg = div_up((size_t)ws.hub_cap * div_up((size_t)dim, (size_t)kWave), (size_t)kWavesPerBlock);
  hipLaunchKernelGGL(csr_hub_combine_kernel, dim3(cg < kHubGridBlocks ? cg : kHubGridBlocks), dim3(kBlock), 0, stream,
                     job, ws, out, dim, out_ld);
}

// The one way to a launch: argument checks (those of launch_block_aggregate: aggregate_args_ok), workspace, row type.
int launch_csr_aggregate(const char *what, bool h_f16, const uint32_t *indptr, const uint32_t *indices,
                         const float *edge_weight, const uint32_t *nodes, size_t first, size_t num_rows,
                         size_t max_edges, const void *h, size_t h_ld, size_t dim, float *out, size_t out_ld,
                         const float *src_deg, int src_mode, const float *dst_deg, int dst_mode, void *ws,
                         size_t ws_bytes, void *stream) {
  if (num_rows == 0) return FGNN_OK;
  if (!indptr || !indices || !float_aligned(indptr) || !float_aligned(indices) || !float_aligned(nodes) ||
      !aggregate_args_ok(h_f16, h, h_ld, dim, out, out_ld, edge_weight, src_deg, src_mode, dst_deg, dst_mode, true))
    return FGNN_EINVAL;
  if (!csr_rows_in_range(nodes != nullptr, first, num_rows, max_edges)) return FGNN_EINVAL;
  const CsrWsLayout l = csr_ws_layout(num_rows, max_edges, dim);
  if (!csr_ws_ok(l, ws, ws_bytes)) return FGNN_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CsrWs w = csr_ws_view(l, ws);
  if (l.bytes) FGNN_HIP_CHECK(hipMemsetAsync(w.counts, 0, 16, s));
  const CsrJob job{indptr, indices, nodes, edge_weight, src_deg, dst_deg, (uint32_t)first, src_mode, dst_mode};
  if (!h_f16) launch_csr<float>(job, w, h, out, num_rows, (uint32_t)dim, (uint32_t)h_ld, (uint32_t)out_ld, s);
  else if (half_rows_paired(h, h_ld, dim))
    launch_csr<__half2>(job, w, h, out, num_rows, (uint32_t)dim, (uint32_t)h_ld, (uint32_t)out_ld, s);
  else launch_csr<__half>(job, w, h, out, num_rows, (uint32_t)dim, (uint32_t)h_ld, (uint32_t)out_ld, s);
  return launch_status(what);
}

}  // namespace
}  // namespace fgnn

extern "C" size_t fgnn_csr_split_length(void) { return fgnn::kCsrSplit; }

extern "C" size_t fgnn_csr_aggregate_workspace_bytes(size_t num_rows, size_t max_edges, size_t dim) {
  return fgnn::csr_ws_layout(num_rows, max_edges, dim).bytes;
}

extern "C" int fgnn_csr_aggregate(const uint32_t *indptr, const uint32_t *indices, const float *edge_weight,
                                  const uint32_t *nodes, size_t first, size_t num_rows, size_t max_edges, const float *h,
                                  size_t h_ld, size_t dim, float *out, size_t out_ld, const float *src_deg, int src_mode,
                                  const float *dst_deg, int dst_mode, void *ws, size_t ws_bytes, void *stream) {
  return fgnn::launch_csr_aggregate(__func__, false, indptr, indices, edge_weight, nodes, first, num_rows, max_edges, h,
                                    h_ld, dim, out, out_ld, src_deg, src_mode, dst_deg, dst_mode, ws, ws_bytes, stream);
}

extern "C" int fgnn_csr_aggregate_f16(const uint32_t *indptr, const uint32_t *indices, const float *edge_weight,
                                      const uint32_t *nodes, size_t first, size_t num_rows, size_t max_edges,
                                      const void *h, size_t h_ld, size_t dim, float *out, size_t out_ld,
                                      const float *src_deg, int src_mode, const float *dst_deg, int dst_mode, void *ws,
                                      size_t ws_bytes, void *stream) {
  return fgnn::launch_csr_aggregate(__func__, true, indptr, indices, edge_weight, nodes, first, num_rows, max_edges, h,
                                    h_ld, dim, out, out_ld, src_deg, src_mode, dst_deg, dst_mode, ws, ws_bytes, stream);
}
