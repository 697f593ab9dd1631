// csr_queue.h -- what the kernels over whole CSR rows share (csr_aggregate.hip: weighted sums; csr_gat_attention.hip:
// edge-softmax attention): the piece length, the workspace of a call (device-side counters, the hub queue, one
// descriptor and one partial row per piece), the row pass's append to that queue, and the range checks of a call.
// A row is cut into pieces of kCsrSplit edges (the last one shorter).  Rows of one piece, and rows the workspace has no
// room for, are computed by their owner wave; longer rows -- the hubs of a power-law graph -- are appended to the queue
// by the row pass (the queue order varies from run to run), their pieces computed into partial rows by the waves of a
// second launch and combined in piece order by a third.
#pragma once
#include "fgnn_device.h"

namespace fgnn {

constexpr uint32_t kCsrSplit = 1024;          // edges of a piece
constexpr uint32_t kNoRow = 0xFFFFFFFFu;      // queue entry / piece descriptor of a hub that found no room
constexpr size_t kHubGridBlocks = 2048;       // hub passes: at most 8 workgroups per CU, strided over the work

// The workspace of a call: counters (zeroed by the call), the hub queue, one descriptor and one partial row per piece.
// Capacities are upper bounds from (num_rows, max_edges): a hub has more than kCsrSplit edges, and ceil(L / kCsrSplit)
// <= L / kCsrSplit + 1 pieces.
struct CsrWs {
  uint32_t *counts;   // [4]: hubs queued, pieces handed out, unused
  uint2 *hubs;        // [hub_cap]   {output row, first piece}
  uint2 *pieces;      // [piece_cap] {output row, piece of that row}
  float *partial;     // [piece_cap][dim]
  uint32_t hub_cap, piece_cap;
};
struct CsrWsLayout { size_t hub_cap, piece_cap, hubs_at, pieces_at, partial_at, bytes; };
inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
// dim: floats of a partial row
inline CsrWsLayout csr_ws_layout(size_t num_rows, size_t max_edges, size_t dim) {
  CsrWsLayout l{};
  const size_t by_edges = max_edges / ((size_t)kCsrSplit + 1);
  l.hub_cap = num_rows < by_edges ? num_rows : by_edges;
  if (l.hub_cap == 0) return l;  // no row of the call can be a hub: no workspace
  l.piece_cap = max_edges / kCsrSplit + l.hub_cap;
  l.hubs_at = 16;
  l.pieces_at = l.hubs_at + round16(l.hub_cap * sizeof(uint2));
  l.partial_at = l.pieces_at + round16(l.piece_cap * sizeof(uint2));
  l.bytes = l.partial_at + l.piece_cap * dim * sizeof(float);
  return l;
}
// does the caller's workspace hold this layout (nothing is needed where no row can be a hub)?
inline bool csr_ws_ok(const CsrWsLayout &l, const void *ws, size_t ws_bytes) {
  if (l.bytes && (!ws || ws_bytes < l.bytes || (reinterpret_cast<uintptr_t>(ws) & 15u) != 0)) return false;
  return fits_u32(l.piece_cap);
}
inline CsrWs csr_ws_view(const CsrWsLayout &l, void *ws) {
  if (!l.bytes) return CsrWs{nullptr, nullptr, nullptr, nullptr, 0, 0};
  char *base = static_cast<char *>(ws);
  return CsrWs{reinterpret_cast<uint32_t *>(base), reinterpret_cast<uint2 *>(base + l.hubs_at),
               reinterpret_cast<uint2 *>(base + l.pieces_at), reinterpret_cast<float *>(base + l.partial_at),
               (uint32_t)l.hub_cap, (uint32_t)l.piece_cap};
}
// output rows are 32-bit in the queue (kNoRow is no row), node ids are 32-bit, edge positions too
inline bool csr_rows_in_range(bool has_nodes, size_t first, size_t num_rows, size_t max_edges) {
  return num_rows < kNoRow && fits_u32(max_edges) &&
         (has_nodes || (fits_u32(first) && first + num_rows <= 0x100000000ull)) &&
         div_up(num_rows, (size_t)kWavesPerBlock) <= 0x7fffffffull;
}

__device__ __forceinline__ uint32_t piece_count(uint32_t len) { return len ? (len - 1) / kCsrSplit + 1 : 1; }

// Row pass, whole wave: output row i of np > 1 pieces asks for a queue entry and np descriptors.  True: the hub passes
// compute the row; false: the workspace has no room, the owner wave computes it.  Every queue entry and descriptor
// below the counters (clamped to the capacities) is written, valid or not.
__device__ __forceinline__ bool csr_queue_hub(const CsrWs &ws, uint32_t i, uint32_t np, uint32_t lane) {
  uint32_t slot = 0, base = 0;
  if (lane == 0) {
    slot = atomicAdd(&ws.counts[0], 1u);
    base = atomicAdd(&ws.counts[1], np);
  }
  slot = __shfl(slot, 0, kWave);
  base = __shfl(base, 0, kWave);
  const bool fits = slot < ws.hub_cap && base < ws.piece_cap && np <= ws.piece_cap - base;
  if (lane == 0 && slot < ws.hub_cap) ws.hubs[slot] = fits ? make_uint2(i, base) : make_uint2(kNoRow, 0u);
  if (base < ws.piece_cap) {
    const uint32_t room = ws.piece_cap - base, wr = np < room ? np : room;
    for (uint32_t k = lane; k < wr; k += kWave) ws.pieces[base + k] = make_uint2(fits ? i : kNoRow, k);
  }
  return fits;
}

}  // namespace fgnn
