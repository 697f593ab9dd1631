// q8_rows.hip -- the kernels of the 8-bit feature store (`feat_store_dtype = q8`; the row format: q8_rows.h): the
// quantiser, the decode, and first-layer aggregation that reads the 8-bit rows as they are -- over sampled blocks
// (the contract of fgnn_block_aggregate_ex / _scaled) and over whole CSR rows (the contract of fgnn_csr_aggregate).
// Sub-wave groups.  block_aggregate_kernel's mapping (one or two columns per lane, 64 lanes per row) would leave most of
// a wave idle on a 144-byte row and fetch the header in a dependent second load.  Here a GROUP of 16 lanes owns one
// edge's row and every lane loads 16 bytes (one dwordx4, sixteen codes): a group load covers 256 contiguous bytes of a
// row, a wave instruction fetches four edges' rows.  For S <= 256 (D <= 240) the header arrives in the same load as the
// codes -- it is the row's last 16 bytes, lane (S - 16) / 16 of the group -- and is broadcast inside the group by
// shuffle; wider rows are walked in passes of 256 bytes of codes, the 8 header bytes fetched once per edge and pass by
// a load of their own (one address per group).  Four group loads are in flight per lane.
// Arithmetic.  Per edge a = (w f_src) scale and b = (w f_src) lo, once per group; per column acc_j = fma(a, q_j, acc_j)
// (byte-to-float conversion, one rounding), and sum_b += b once per edge: sum_b is added to every column when the
// segment is flushed.  A lane holds 16 fp32 accumulators; no dequantised row is ever written.
// Sampled blocks: a wave takes a chunk of 64 edges (lane i holds edge i), group g the 16 CONSECUTIVE edges 16 g ..
// 16 g + 15 of it -- consecutive rather than every fourth, so that a destination's run is cut into as few segments as
// possible: blocks with a handful of edges per destination are bound by the flush's atomics.  Every group keeps its own
// current destination and flushes its own segment with float atomics; before that the accumulators are transposed
// inside the group (16 x 16, four butterfly stages) so that an atomic instruction touches 16 consecutive columns per
// group instead of every sixteenth.  Sums in fp32, the order of the additions is not fixed; against the float64 sum over
// the exactly decoded rows every output stays within (2 k + 8) 2^-23 of the sum of its terms' magnitudes, both halves
// |w f scale q| and |w f lo| of every affine term counted, k = the destination's edge count (tests/test_q8_kernels_gpu.py).
// CSR rows: one wave owns an output row; edge i of a piece goes to group i mod 4; a group adds its edges in CSR order
// from 0 (acc_j and sum_b, then acc_j + sum_b); the four group sums combine as (g0 + g1) + (g2 + g3); pieces of kCsrSplit
// edges combine in piece order from 0; the destination factor multiplies once.  No float atomics, out overwritten,
// zeros for an empty row, long rows through csr_queue.h's queue / partial / combine scheme with fgnn_csr_aggregate's
// workspace.  The order differs from the fp32 kernel's; the promise is the same: a row's bits depend on the row and D
// only.
#include "q8_rows.h"
#include "csr_queue.h"

namespace fgnn {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kQ8EdgesPerWave = kWave;                            // sampled blocks: lane i holds edge i
constexpr uint32_t kQ8EdgesPerGroup = kQ8EdgesPerWave / kQ8Groups;     // 16 consecutive edges
constexpr uint32_t UN = 4;                                             // group loads in flight per lane

__device__ __forceinline__ uint32_t row_bytes(uint32_t dim) { return ((dim + 15u) & ~15u) + 16u; }
__device__ __forceinline__ uint4 load16(const unsigned char *p) { return *reinterpret_cast<const uint4 *>(p); }
__host__ __device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// 16 x 16 transpose inside a group: afterwards lane s of the group holds in r[t] what lane t held in r[s].  Stage m
// swaps bit m of the lane with bit m of the register index; every register index is a compile-time constant.
__device__ __forceinline__ void transpose16(float (&r)[16], uint32_t sub) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) {
    const bool upper = (sub & (uint32_t)m) != 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i & m) continue;
      const float a = r[i], b = r[i | m];  // (both registers are written: a store under a condition would index them)
      const float recv = __shfl_xor(upper ? a : b, m, kWave);
      r[i] = upper ? recv : a;
      r[i | m] = upper ? b : recv;
    }
  }
}

// One edge's share of a row for the pass whose lane offset is `off`: the lane's sixteen codes and the header {scale, lo}.
// INLINE (S <= 256): the header is in the group load itself, the row's last 16 bytes.  Masked lanes and edges load
// nothing.
template <bool INLINE>
__device__ __forceinline__ void fetch_edge(uint4 &v, float2 &hd, const unsigned char *rp, uint32_t off, uint32_t codes,
                                           bool lane_on, bool edge_on) {
  v = (lane_on && edge_on) ? load16(rp + off) : make_uint4(0u, 0u, 0u, 0u);
  hd = make_float2(0.0f, 0.0f);
  if constexpr (!INLINE) {
    if (edge_on) hd = *reinterpret_cast<const float2 *>(rp + codes);
  }
}
// the edge's header; call with the whole group active.  hdr_lane: the wave lane that loaded the row's last 16 bytes.
template <bool INLINE>
__device__ __forceinline__ float2 edge_header(const uint4 &v, const float2 &hd, int hdr_lane) {
  if constexpr (INLINE)
    return make_float2(__uint_as_float(__shfl(v.x, hdr_lane, kWave)), __uint_as_float(__shfl(v.y, hdr_lane, kWave)));
  else return hd;
}

// ---- sampled blocks ---------------------------------------------------------------------------------------------------
// SCALED: lane i's weight is multiplied by its source's degree factor and the destination factor of its segment travels
// beside it, as in block_aggregate_kernel.  All lanes run the edge loop with the trip count of group 0 (the fullest);
// a group's own edges are masked by n_g, memory operations by the lane's byte offset.
template <bool SCALED, bool INLINE>
__global__ __launch_bounds__(kBlock) void q8_block_aggregate_kernel(
    const uint32_t *__restrict__ src_idx, const uint32_t *__restrict__ dst_idx, const float *__restrict__ w,
    const unsigned char *__restrict__ h, float *out, size_t num_edge, uint32_t dim, uint32_t h_ld, uint32_t out_ld,
    float *deg, const float *__restrict__ src_deg, int src_mode, const float *__restrict__ dst_deg, int dst_mode) {
  const size_t wave = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  const size_t e0 = wave * kQ8EdgesPerWave;
  if (e0 >= num_edge) return;  // wave-uniform
  const uint32_t cnt = num_edge - e0 < kQ8EdgesPerWave ? (uint32_t)(num_edge - e0) : kQ8EdgesPerWave;
  const uint32_t lane = (uint32_t)lane_id(), sub = lane & (kQ8Group - 1), first = lane & ~(kQ8Group - 1);
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
  // in-degrees on the way, as block_aggregate_kernel counts them: one float atomic per (wave, run of equal destinations)
  if (deg) {
    const uint32_t prev = __shfl_up(my_dst, 1, kWave);
    const bool head = lane < cnt && (lane == 0 || prev != my_dst);
    const unsigned long long heads = __ballot(head);
    if (head) unsafeAtomicAdd(&deg[my_dst], (float)run_length_at_head(heads, lane, cnt));
  }
  const uint32_t S = row_bytes(dim), codes = S - 16;
  const uint32_t n_g = cnt > first ? (cnt - first < kQ8EdgesPerGroup ? cnt - first : kQ8EdgesPerGroup) : 0;  // group-uniform
  const uint32_t n_0 = cnt < kQ8EdgesPerGroup ? cnt : kQ8EdgesPerGroup;                                      // wave-uniform
  const int hdr_lane = (int)(first + codes / kQ8LaneBytes);  // INLINE only
  for (uint32_t pbase = 0; pbase < codes; pbase += kQ8PassBytes) {  // one trip for D <= 256
    const uint32_t off = pbase + kQ8LaneBytes * sub;
    const bool lane_on = off < (INLINE ? S : codes);
    float acc[16], sum_b = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
    uint32_t cur = __shfl(my_dst, (int)first, kWave);
    [[maybe_unused]] float cur_fd = 1.0f;
    if constexpr (SCALED) cur_fd = __shfl(my_fd, (int)first, kWave);
    // the flush of a group's segment (group-uniform): sum_b joins every column, the destination factor multiplies once,
    // the sums change lanes (values moved, not changed) and instruction t adds the group's columns 16 t .. 16 t + 15
    auto flush = [&](uint32_t dst) {
      float r[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        r[j] = acc[j] + sum_b;
        if constexpr (SCALED) r[j] = cur_fd * r[j];
        acc[j] = 0.0f;
      }
      sum_b = 0.0f;
      transpose16(r, sub);
      float *op = out + (size_t)dst * out_ld + pbase + sub;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        if (pbase + kQ8Group * t + sub < dim) unsafeAtomicAdd(op + kQ8Group * t, r[t]);
      }
    };
    for (uint32_t i0 = 0; i0 < n_0; i0 += UN) {
      uint4 v[UN];
      float2 hd[UN];
      uint32_t c[UN];
      float we[UN];
      [[maybe_unused]] float fd[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const bool edge_on = i0 + u < n_g;
        const int li = (int)(first + (edge_on ? i0 + u : 0u));
        const uint32_t sidx = __shfl(my_src, li, kWave);
        c[u] = __shfl(my_dst, li, kWave);
        we[u] = __shfl(my_w, li, kWave);
        if constexpr (SCALED) fd[u] = __shfl(my_fd, li, kWave);
        fetch_edge<INLINE>(v[u], hd[u], h + (size_t)sidx * h_ld, off, codes, lane_on, edge_on);
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (i0 + u < n_g) {  // group-uniform
          const float2 sl = edge_header<INLINE>(v[u], hd[u], hdr_lane);
          if (c[u] != cur) {  // group-uniform: segment boundary
            flush(cur);
            cur = c[u];
            if constexpr (SCALED) cur_fd = fd[u];
          }
          q8_fma16(acc, v[u], we[u] * sl.x);
          sum_b += we[u] * sl.y;
        }
      }
    }
    if (n_g) flush(cur);
  }
}

int launch_q8_block_aggregate(const char *what, bool scaled, const uint32_t *src_index, const uint32_t *dst_index,
                              const float *edge_weight, size_t num_edge, const void *h, size_t h_ld, size_t dim,
                              float *out, size_t out_ld, float *in_degree, const float *src_deg, int src_mode,
                              const float *dst_deg, int dst_mode, void *stream) {
  if (num_edge == 0) return FGNN_OK;
  if (!src_index || !dst_index || !float_aligned(src_index) || !float_aligned(dst_index) || !float_aligned(in_degree) ||
      !q8_aggregate_args_ok(h, h_ld, dim, out, out_ld, edge_weight, src_deg, src_mode, dst_deg, dst_mode))
    return FGNN_EINVAL;
  const size_t blocks = div_up(div_up(num_edge, (size_t)kQ8EdgesPerWave), (size_t)kWavesPerBlock);
  if (blocks > 0x7fffffffull) return FGNN_EINVAL;
  using Kernel = decltype(&q8_block_aggregate_kernel<false, false>);
  static constexpr Kernel kernels[2][2] = {
      {q8_block_aggregate_kernel<false, false>, q8_block_aggregate_kernel<false, true>},
      {q8_block_aggregate_kernel<true, false>, q8_block_aggregate_kernel<true, true>}};
  hipLaunchKernelGGL(kernels[scaled][q8_row_bytes(dim) <= kQ8PassBytes], dim3(blocks), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), src_index, dst_index, edge_weight,
                     static_cast<const unsigned char *>(h), out, num_edge, (uint32_t)dim, (uint32_t)h_ld,
                     (uint32_t)out_ld, in_degree, src_deg, src_mode, dst_deg, dst_mode);
  return launch_status(what);
}

// ---- whole CSR rows ---------------------------------------------------------------------------------------------------
struct Q8Job {
  const uint32_t *indptr, *indices, *nodes;
  const float *w, *src_deg, *dst_deg;
  uint32_t first;
  int src_mode, dst_mode;
};
__device__ __forceinline__ uint32_t job_node(const Q8Job &j, size_t i) { return j.nodes ? j.nodes[i] : j.first + (uint32_t)i; }
// dst_deg == null: the row's own length is the degree
__device__ __forceinline__ float job_dst_factor(const Q8Job &j, uint32_t v, uint32_t len) {
  return j.dst_mode ? degree_factor(j.dst_deg ? j.dst_deg[v] : (float)len, j.dst_mode) : 1.0f;
}

// val[j] = the sum of the cnt (<= kCsrSplit) edges from position p0 on for columns pbase + 16 sub + j, the same bits in
// all four groups.  The wave's lanes load 64 neighbour ids (and weights) at a time, coalesced; group g takes the edges
// g, g + 4, ... of those 64 in CSR order: the group is decided by the edge's index inside the piece, c0 + e, and c0 is a
// multiple of 64 -- edge i of the piece goes to group i mod 4, wherever the row starts in `indices`.
template <bool INLINE>
__device__ __forceinline__ void q8_sum_piece(float (&val)[16], const Q8Job &job, const unsigned char *__restrict__ h,
                                             uint32_t h_ld, uint32_t S, uint32_t pbase, uint32_t p0, uint32_t cnt,
                                             uint32_t lane) {
  const uint32_t sub = lane & (kQ8Group - 1), g = lane / kQ8Group, codes = S - 16;
  const uint32_t off = pbase + kQ8LaneBytes * sub;
  const bool lane_on = off < (INLINE ? S : codes);
  const int hdr_lane = (int)(g * kQ8Group + codes / kQ8LaneBytes);
  float acc[16], sum_b = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
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
    const uint32_t steps = (n + kQ8Groups - 1) / kQ8Groups;  // wave-uniform: group 0's edge count
    for (uint32_t j0 = 0; j0 < steps; j0 += UN) {
      uint4 v[UN];
      float2 hd[UN];
      float we[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t e = kQ8Groups * (j0 + u) + g;
        const bool edge_on = e < n;
        const int li = (int)(edge_on ? e : 0u);
        const uint32_t sidx = __shfl(my_src, li, kWave);
        we[u] = __shfl(my_w, li, kWave);
        fetch_edge<INLINE>(v[u], hd[u], h + (size_t)sidx * h_ld, off, codes, lane_on, edge_on);
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (kQ8Groups * (j0 + u) + g < n) {  // group-uniform
          const float2 sl = edge_header<INLINE>(v[u], hd[u], hdr_lane);
          q8_fma16(acc, v[u], we[u] * sl.x);
          sum_b += we[u] * sl.y;
        }
      }
    }
  }
  // the group's sum, then (g0 + g1) + (g2 + g3): fp32 addition commutes, so both sides of an exchange get the same bits
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float v = acc[j] + sum_b;
    v += __shfl_xor(v, 16, kWave);
    v += __shfl_xor(v, 32, kWave);
    val[j] = v;
  }
}

// Stores scale * val for the 256 columns of pass `pbase` of the row at `op`.  All four groups hold the same sums: group
// g stores columns 16 sub + 4 g .. + 3 of its lane's sixteen, so one wave instruction covers 1024 contiguous bytes.
__device__ __forceinline__ void q8_store_pass(float *op, const float (&val)[16], float scale, uint32_t pbase, uint32_t dim,
                                              uint32_t lane) {
  const uint32_t sub = lane & (kQ8Group - 1), g = lane / kQ8Group;
  float o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float lo2 = (g & 1u) ? val[4 + k] : val[k], hi2 = (g & 1u) ? val[12 + k] : val[8 + k];
    o[k] = scale * ((g & 2u) ? hi2 : lo2);
  }
  const uint32_t col = (pbase + kQ8Group * sub + 4 * g);
  float *p = op + col;
  if (col + 3 < dim && aligned16(p)) {
    *reinterpret_cast<f4 *>(p) = f4{o[0], o[1], o[2], o[3]};
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col + k < dim) p[k] = o[k];
    }
  }
}

// Row pass: wave (blockIdx.x, wave_id) owns output row i; hubs go to the queue where the workspace has room.
// A pass's 256 bytes of codes are 256 columns: byte offset and column offset of a pass are the same number.
template <bool INLINE>
__global__ __launch_bounds__(kBlock) void q8_csr_rows_kernel(Q8Job job, CsrWs ws, const unsigned char *__restrict__ h,
                                                             float *out, size_t num_rows, uint32_t dim, uint32_t h_ld,
                                                             uint32_t out_ld) {
  const size_t i = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  if (i >= num_rows) return;  // wave-uniform
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t v = job_node(job, i);
  const uint32_t beg = job.indptr[v], len = job.indptr[v + 1] - beg;
  const uint32_t np = piece_count(len);
  if (np > 1 && ws.hub_cap && csr_queue_hub(ws, (uint32_t)i, np, lane)) return;  // wave-uniform
  const float fd = job_dst_factor(job, v, len);
  const uint32_t S = row_bytes(dim);
  float *op = out + i * out_ld;
  for (uint32_t pbase = 0; pbase < S - 16; pbase += kQ8PassBytes) {
    float total[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) total[j] = 0.0f;
    for (uint32_t k = 0; k < np; ++k) {
      float val[16];
      const uint32_t done = k * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
      q8_sum_piece<INLINE>(val, job, h, h_ld, S, pbase, beg + done, cnt, lane);
#pragma unroll
      for (int j = 0; j < 16; ++j) total[j] += val[j];
    }
    q8_store_pass(op, total, fd, pbase, dim, lane);
  }
}

// Hub pass 1: every queued piece's sum into its partial row.
template <bool INLINE>
__global__ __launch_bounds__(kBlock) void q8_csr_hub_pieces_kernel(Q8Job job, CsrWs ws, const unsigned char *__restrict__ h,
                                                                   uint32_t dim, uint32_t h_ld) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t handed = ws.counts[1], n = handed < ws.piece_cap ? handed : ws.piece_cap;
  const uint32_t stride = gridDim.x * kWavesPerBlock;
  const uint32_t S = row_bytes(dim);
  for (uint32_t p = blockIdx.x * kWavesPerBlock + wave_id(); p < n; p += stride) {
    const uint2 d = ws.pieces[p];
    if (d.x == kNoRow) continue;  // wave-uniform
    const uint32_t v = job_node(job, d.x);
    const uint32_t beg = job.indptr[v], len = job.indptr[v + 1] - beg;
    const uint32_t done = d.y * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
    float *pp = ws.partial + (size_t)p * dim;
    for (uint32_t pbase = 0; pbase < S - 16; pbase += kQ8PassBytes) {
      float val[16];
      q8_sum_piece<INLINE>(val, job, h, h_ld, S, pbase, beg + done, cnt, lane);
      q8_store_pass(pp, val, 1.0f, pbase, dim, lane);
    }
  }
}

// Hub pass 2: one wave per (queued hub, 64 columns) adds the hub's partial rows in piece order from 0 -- the additions
// the row pass makes for a row it sums itself -- and stores the output row.
__global__ __launch_bounds__(kBlock) void q8_csr_hub_combine_kernel(Q8Job job, CsrWs ws, float *out, uint32_t dim,
                                                                    uint32_t out_ld) {
  constexpr uint32_t UC = 8;
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
    for (uint32_t k0 = 0; k0 < np; k0 += UC) {
      float t[UC];
#pragma unroll
      for (uint32_t u = 0; u < UC; ++u) t[u] = (c < dim && k0 + u < np) ? pp[(size_t)(k0 + u) * dim] : 0.0f;
#pragma unroll
      for (uint32_t u = 0; u < UC; ++u) {
        if (k0 + u >= np) break;  // wave-uniform
        total += t[u];
      }
    }
    if (c < dim) out[(size_t)hub.x * out_ld + c] = job_dst_factor(job, v, len) * total;
  }
}

// zeroes the workspace's four counters (a kernel, not a memset node: the call may be captured into a graph)
__global__ void q8_csr_clear_counts_kernel(uint32_t *counts) {
  if (threadIdx.x < 4) counts[threadIdx.x] = 0u;
}

template <bool INLINE>
void launch_q8_csr(const Q8Job &job, const CsrWs &ws, const unsigned char *h, float *out, size_t num_rows, uint32_t dim,
                   uint32_t h_ld, uint32_t out_ld, hipStream_t stream) {
  hipLaunchKernelGGL(q8_csr_rows_kernel<INLINE>, dim3(div_up(num_rows, (size_t)kWavesPerBlock)), dim3(kBlock), 0, stream,
                     job, ws, h, out, num_rows, dim, h_ld, out_ld);
  if (!ws.hub_cap) return;
  const size_t pg = div_up((size_t)ws.piece_cap, (size_t)kWavesPerBlock);
  hipLaunchKernelGGL(q8_csr_hub_pieces_kernel<INLINE>, dim3(pg < kHubGridBlocks ? pg : kHubGridBlocks), dim3(kBlock), 0,
                     stream, job, ws, h, dim, h_ld);
  const size_t cg = div_up((size_t)ws.hub_cap * div_up((size_t)dim, (size_t)kWave), (size_t)kWavesPerBlock);
  hipLaunchKernelGGL(q8_csr_hub_combine_kernel, dim3(cg < kHubGridBlocks ? cg : kHubGridBlocks), dim3(kBlock), 0, stream,
                     job, ws, out, dim, out_ld);
}

// ---- quantiser ----------------------------------------------------------------------------------------------------------
// One wave per row.  Lane l owns the dwords l, l + 64, ... of the output row (four codes each); the first kHeld of them
// per lane keep their four inputs in registers between the min / max pass and the encode pass -- rows of up to 1024
// columns are read once, the tail of longer rows twice.  The encode, in fp32 IEEE operations in this order (no
// contraction: the file is built with -ffp-contract=off): scale = (hi - lo) / 255, inv = 255 / (hi - lo),
// q = min(255, max(0, rint((x - lo) * inv))), round to nearest even; hi == lo: scale = 0, every code 0.  A NaN is
// skipped by min / max and encodes as 0, an infinity clamps: every index below is independent of the data.
constexpr int kHeld = 4;

// (inv == 0 on a flat row: the product is 0 or NaN, the code 0 either way)
__device__ __forceinline__ uint32_t q8_encode(float x, float lo, float inv) {
  return (uint32_t)fminf(255.0f, fmaxf(0.0f, rintf((x - lo) * inv)));
}

__global__ __launch_bounds__(kBlock) void q8_quantize_kernel(const float *__restrict__ x, uint32_t x_ld, size_t n,
                                                             uint32_t dim, unsigned char *__restrict__ out,
                                                             uint32_t out_ld) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t S = row_bytes(dim), words = S / 4, code_words = words - 4;
  const uint32_t trips = (words + kWave - 1) / kWave;
  for (size_t row = (size_t)blockIdx.x * kWavesPerBlock + wave_id(); row < n; row += (size_t)gridDim.x * kWavesPerBlock) {
    const float *xp = x + row * x_ld;
    uint32_t *op = reinterpret_cast<uint32_t *>(out + row * out_ld);
    float lo = __builtin_inff(), hi = -__builtin_inff();
    // the four inputs of dword wd (columns beyond dim, and dwords beyond the codes, read nothing)
    auto read4 = [&](uint32_t wd, float (&v)[4]) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (wd < code_words && 4 * wd + k < dim) ? xp[4 * wd + k] : 0.0f;
    };
    auto fold4 = [&](uint32_t wd, const float (&v)[4]) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (wd < code_words && 4 * wd + k < dim) {
          lo = fminf(lo, v[k]);
          hi = fmaxf(hi, v[k]);
        }
      }
    };
    float held[kHeld][4];
#pragma unroll
    for (int t = 0; t < kHeld; ++t) {
      read4(lane + kWave * t, held[t]);
      fold4(lane + kWave * t, held[t]);
    }
    for (uint32_t t = kHeld; t < trips; ++t) {
      float v[4];
      read4(lane + kWave * t, v);
      fold4(lane + kWave * t, v);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, d, kWave));
      hi = fmaxf(hi, __shfl_xor(hi, d, kWave));
    }
    const bool flat = hi == lo;
    const float scale = flat ? 0.0f : (hi - lo) / 255.0f, inv = flat ? 0.0f : 255.0f / (hi - lo);
    // every dword of [0, S): codes (zero beyond dim), then scale, lo, and two zero words
    auto write4 = [&](uint32_t wd, const float (&v)[4]) {
      if (wd >= words) return;
      uint32_t word = 0u;
      if (wd < code_words) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (4 * wd + k < dim) word |= q8_encode(v[k], lo, inv) << (8 * k);
        }
      } else if (wd == code_words) {
        word = __float_as_uint(scale);
      } else if (wd == code_words + 1) {
        word = __float_as_uint(lo);
      }
      op[wd] = word;
    };
#pragma unroll
    for (int t = 0; t < kHeld; ++t) write4(lane + kWave * t, held[t]);
    for (uint32_t t = kHeld; t < trips; ++t) {
      float v[4];
      read4(lane + kWave * t, v);
      write4(lane + kWave * t, v);
    }
  }
}

// ---- decode -------------------------------------------------------------------------------------------------------------
// One thread per (row, four columns): a dword of codes and the row's header in, four fp32 out (one 16-byte store where
// the address allows).  out = q8_decode(scale, lo, q): one multiply, one add, not fused.
__device__ __forceinline__ void q8_decode4(const unsigned char *rp, uint32_t S, uint32_t c, float (&v)[4]) {
  const uint32_t word = *reinterpret_cast<const uint32_t *>(rp + c);
  const float2 hd = *reinterpret_cast<const float2 *>(rp + S - 16);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = q8_decode(hd.x, hd.y, q8_code(word, k));
}

__global__ __launch_bounds__(kBlock) void q8_dequantize_kernel(const unsigned char *__restrict__ h, uint32_t h_ld,
                                                               const uint32_t *__restrict__ index, size_t n, uint32_t dim,
                                                               float *__restrict__ out, uint32_t out_ld) {
  const uint32_t q = (dim + 3) / 4, S = row_bytes(dim);
  const size_t total = n * q;
  for (size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (size_t)gridDim.x * kBlock) {
    const size_t i = t / q;
    const uint32_t c = (uint32_t)(t - i * q) * 4;
    const size_t r = index ? index[i] : i;
    float v[4];
    q8_decode4(h + r * h_ld, S, c, v);
    float *p = out + i * out_ld + c;
    if (c + 3 < dim && aligned16(p)) {
      *reinterpret_cast<f4 *>(p) = f4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (c + k < dim) p[k] = v[k];
      }
    }
  }
}

// fgnn_sage_finish_z over q8 rows: z[:, :din] = decode(h[:num_dst]), inv = 1 / max(deg, 1), z[:, din:] *= inv
// (sage_finish_z_kernel's thread mapping: din % 4 == 0, 16-byte aligned rows of z)
__global__ __launch_bounds__(kBlock) void q8_sage_finish_z_kernel(float *__restrict__ z, uint32_t ld,
                                                                  const unsigned char *__restrict__ h, uint32_t h_ld,
                                                                  const float *__restrict__ deg, float *__restrict__ inv_out,
                                                                  uint32_t num_dst, uint32_t din) {
  const uint32_t q = din / 4, S = row_bytes(din);
  const size_t total = (size_t)num_dst * q;
  for (size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (size_t)gridDim.x * kBlock) {
    const uint32_t i = (uint32_t)(t / q), c = (uint32_t)(t - (size_t)i * q) * 4;
    const float d = deg[i];
    const float inv = 1.0f / (d < 1.0f ? 1.0f : d);
    if (c == 0) inv_out[i] = inv;
    float v[4];
    q8_decode4(h + (size_t)i * h_ld, S, c, v);
    *reinterpret_cast<f4 *>(z + (size_t)i * ld + c) = f4{v[0], v[1], v[2], v[3]};
    f4 *zr = reinterpret_cast<f4 *>(z + (size_t)i * ld + din + c);
    f4 r = *zr;
    r.x *= inv; r.y *= inv; r.z *= inv; r.w *= inv;
    *zr = r;
  }
}

// grid of a kernel that walks `total` items with a stride: enough workgroups to fill the device, no more
size_t strided_blocks(size_t total, size_t per_block) {
  const size_t blocks = div_up(total, per_block), most = (size_t)device_cu_count() * 16;
  return blocks < most ? blocks : most;
}

}  // namespace
}  // namespace fgnn

using namespace fgnn;

extern "C" size_t fgnn_q8_row_bytes(size_t dim) { return q8_row_bytes(dim); }

extern "C" int fgnn_quantize_rows_q8(const float *x, size_t x_ld, size_t num_rows, size_t dim, void *out, size_t out_ld,
                                     void *stream) {
  if (num_rows == 0) return FGNN_OK;
  if (!x || !float_aligned(x) || x_ld < dim || !fits_u32(x_ld) || !q8_rows_ok(out, out_ld, dim)) return FGNN_EINVAL;
  hipLaunchKernelGGL(q8_quantize_kernel, dim3(strided_blocks(num_rows, kWavesPerBlock)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), x, (uint32_t)x_ld, num_rows, (uint32_t)dim,
                     static_cast<unsigned char *>(out), (uint32_t)out_ld);
  return launch_status(__func__);
}

extern "C" int fgnn_dequantize_rows_q8(const void *h, size_t h_ld, const uint32_t *index, size_t num_rows, size_t dim,
                                       float *out, size_t out_ld, void *stream) {
  if (num_rows == 0) return FGNN_OK;
  if (!q8_rows_ok(h, h_ld, dim) || !out || !float_aligned(out) || !float_aligned(index) || out_ld < dim ||
      !fits_u32(out_ld))
    return FGNN_EINVAL;
  hipLaunchKernelGGL(q8_dequantize_kernel, dim3(strided_blocks(num_rows * div_up(dim, (size_t)4), kBlock)), dim3(kBlock),
                     0, static_cast<hipStream_t>(stream), static_cast<const unsigned char *>(h), (uint32_t)h_ld, index,
                     num_rows, (uint32_t)dim, out, (uint32_t)out_ld);
  return launch_status(__func__);
}

extern "C" int fgnn_block_aggregate_ex_q8(const uint32_t *src_index, const uint32_t *dst_index, const float *edge_weight,
                                          size_t num_edge, const void *h, size_t h_ld, size_t dim, float *out,
                                          size_t out_ld, float *in_degree, void *stream) {
  return launch_q8_block_aggregate(__func__, false, src_index, dst_index, edge_weight, num_edge, h, h_ld, dim, out, out_ld,
                                   in_degree, nullptr, 0, nullptr, 0, stream);
}

extern "C" int fgnn_block_aggregate_scaled_q8(const uint32_t *src_index, const uint32_t *dst_index,
                                              const float *edge_weight, size_t num_edge, const void *h, size_t h_ld,
                                              size_t dim, float *out, size_t out_ld, const float *src_deg, int src_mode,
                                              const float *dst_deg, int dst_mode, void *stream) {
  return launch_q8_block_aggregate(__func__, true, src_index, dst_index, edge_weight, num_edge, h, h_ld, dim, out, out_ld,
                                   nullptr, src_deg, src_mode, dst_deg, dst_mode, stream);
}

extern "C" int fgnn_sage_finish_z_q8(float *z, size_t ld, const void *h, size_t h_ld, const float *deg, float *inv,
                                     size_t num_dst, size_t din, void *stream) {
  if (num_dst == 0) return FGNN_OK;
  if (!z || !deg || !inv || din == 0 || din % 4 || ld < 2 * din || ld % 4 || !fits_u32(num_dst) || !fits_u32(ld) ||
      !q8_rows_ok(h, h_ld, din) || !aligned16(z) || !float_aligned(deg) || !float_aligned(inv))
    return FGNN_EINVAL;
  hipLaunchKernelGGL(q8_sage_finish_z_kernel, dim3(strided_blocks(num_dst * (din / 4), kBlock)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), z, (uint32_t)ld, static_cast<const unsigned char *>(h),
                     (uint32_t)h_ld, deg, inv, (uint32_t)num_dst, (uint32_t)din);
  return launch_status(__func__);
}

extern "C" int fgnn_csr_aggregate_q8(const uint32_t *indptr, const uint32_t *indices, const float *edge_weight,
                                     const uint32_t *nodes, size_t first, size_t num_rows, size_t max_edges,
                                     const void *h, size_t h_ld, size_t dim, float *out, size_t out_ld,
                                     const float *src_deg, int src_mode, const float *dst_deg, int dst_mode, void *ws,
                                     size_t ws_bytes, void *stream) {
  if (num_rows == 0) return FGNN_OK;
  if (!indptr || !indices || !float_aligned(indptr) || !float_aligned(indices) || !float_aligned(nodes) ||
      !q8_aggregate_args_ok(h, h_ld, dim, out, out_ld, edge_weight, src_deg, src_mode, dst_deg, dst_mode, true))
    return FGNN_EINVAL;
  if (!csr_rows_in_range(nodes != nullptr, first, num_rows, max_edges)) return FGNN_EINVAL;
  const CsrWsLayout l = csr_ws_layout(num_rows, max_edges, dim);
  if (!csr_ws_ok(l, ws, ws_bytes)) return FGNN_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CsrWs w = csr_ws_view(l, ws);
  if (l.bytes) hipLaunchKernelGGL(q8_csr_clear_counts_kernel, dim3(1), dim3(kWave), 0, s, w.counts);
  const Q8Job job{indptr, indices, nodes, edge_weight, src_deg, dst_deg, (uint32_t)first, src_mode, dst_mode};
  const unsigned char *hp = static_cast<const unsigned char *>(h);
  if (q8_row_bytes(dim) <= kQ8PassBytes)
    launch_q8_csr<true>(job, w, hp, out, num_rows, (uint32_t)dim, (uint32_t)h_ld, (uint32_t)out_ld, s);
  else launch_q8_csr<false>(job, w, hp, out, num_rows, (uint32_t)dim, (uint32_t)h_ld, (uint32_t)out_ld, s);
  return launch_status(__func__);
}
