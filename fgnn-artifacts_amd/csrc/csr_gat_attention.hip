// csr_gat_attention.hip -- a GAT layer's attention aggregation over whole CSR rows: the message-passing step of exact
// layer-wise GAT inference on the full graph (examples/inference.py: gat_layerwise_inference).  H heads of F features,
// D = H F; for output row i, v = nodes ? nodes[i] : first + i, over p in [indptr[v], indptr[v + 1]):
//     s[p,h] = leaky_relu(el[indices[p],h] + er[v,h])     a[p,h] = softmax of s[.,h] over the row
//     out[i,h,:] = sum_p a[p,h] feat[indices[p],h,:]
// gat_attention.hip serves sampled COO blocks and training: a destination per edge, E x H scores and E x H alphas in
// scratch, a pre-filled output, float atomics for the per-destination max and sums.  A CSR row needs none of that: its
// edges are one contiguous run, so ONE wave owns the output row, keeps max, sum and weighted sums in registers and stores
// once -- csr_aggregate.hip's shape, whose queue of long rows this file shares (csr_queue.h).  out is overwritten, a row
// without a neighbour writes zeros, er is indexed by NODE id, there is no dropout, no alpha output, no atomic on a
// float.  fp32 only.
// The order of the operations is fixed by the row alone.  A row is cut into pieces of kCsrSplit edges; piece k has
//     m_k[h] = max of its scores (exact in any order)
//     z_k[h] = 0 + exp(s - m_k) ...           in CSR order
//     acc_k  = 0 + exp(s - m_k) feat ...      in CSR order
// and the row combines its pieces in piece order: m = max_k m_k, c_k = exp(m_k - m), Z = 0 + c_k z_k ..., A = 0 +
// c_k acc_k ..., out = A / Z.  A row of one piece has c_0 = exp(0) = 1: short and long rows obey one definition.  Who
// computes a piece does not enter: rows of one piece and rows the workspace has no room for are computed by their owner
// wave, longer rows are queued by the row pass, their pieces left as (acc_k | z_k | m_k) in partial rows by a second
// launch and combined by a third.  So a node's result is bit for bit the same in a call over [0, N) and in a call over
// 7 nodes.  Three stream-ordered launches (one where no row can be a hub), one 16-byte memset, no host synchronisation.
// Inside a piece: the wave's lanes load 64 neighbour ids at a time, coalesced, and each computes its edge's H scores.
// Lane l owns columns l + 64 q (a pass of 64 P columns, a dbase loop beyond 256); the weight of column c is that of
// head c / F.  Getting edge i's weight of head c / F to the lane that owns column c is what the LDS is for: the chunk's
// 64 x H weights are STAGED IN LDS PER WAVE (stage[edge][head], 64 x kMaxHeads floats = 4 KiB per wave, 16 KiB per
// workgroup of 4 waves -- ten workgroups per CU by LDS, more than the 8 the wave slots hold, so the LDS does not bound
// occupancy), written by the edge's lane and read back as stage[i][head of my column]: the lanes of a slot read at most
// ceil(64 / F) + 1 distinct addresses, the rest is broadcast.  No register array is indexed dynamically.  The same
// staging holds the chunk's scores for the max: lane l takes head l % Hp (Hp = H rounded up to a power of two) of the
// edges l / Hp + (64 / Hp) j, conflict-free for H a power of two, then xor shuffles.  Only the owning wave touches its
// staging: the wave's LDS operations execute in order, a wavefront-scope fence keeps the compiler from reordering them.
// H <= kMaxHeads = 16 (fgnn_csr_gat_max_heads); a larger H is refused with FGNN_EINVAL.
// A piece of at most 64 edges (nearly every row of a graph with 15 edges per row) computes its scores once: they stay
// staged between the max and the sums; longer pieces compute each score twice (el is re-read, from L2 mostly) rather
// than keep 1024 x H of them.
// Index widths as in csr_aggregate.hip: edge positions and node ids are uint32_t, every address into feat, el, er, out
// and the partial rows is formed in size_t.
#include "csr_queue.h"

namespace fgnn {
namespace {

constexpr uint32_t kMaxHeads = 16;  // heads the per-wave staging holds

// The graph, the rows asked for and the layer's projections: what all three kernels read.
struct GatJob {
  const uint32_t *indptr, *indices, *nodes;
  const float *el, *er, *feat;
  uint32_t first, H, F, dim, feat_ld;
  float slope;
};
__device__ __forceinline__ uint32_t job_node(const GatJob &j, size_t i) { return j.nodes ? j.nodes[i] : j.first + (uint32_t)i; }
__device__ __forceinline__ uint32_t pow2_heads(uint32_t H) { return H <= 1 ? 1u : 1u << (32 - __builtin_clz(H - 1)); }

// orders the wave's own LDS writes and reads (different lanes, same wave) for the compiler; the hardware runs a wave's
// LDS operations in order
__device__ __forceinline__ void stage_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// stage[lane][h] = the score of edge p0 + lane towards v for every head (lanes >= n stage nothing)
__device__ __forceinline__ void stage_scores(float *stage, const GatJob &job, uint32_t v, uint32_t src, bool live,
                                             uint32_t lane) {
  if (!live) return;
  const float *lp = job.el + (size_t)src * job.H, *rp = job.er + (size_t)v * job.H;
  for (uint32_t h = 0; h < job.H; ++h) {
    const float x = lp[h] + rp[h];
    stage[lane * job.H + h] = x > 0.0f ? x : job.slope * x;
  }
}

// m_k: lane l returns the max of head l % Hp over the cnt (<= kCsrSplit) edges from position p0 on (-inf for l % Hp >=
// H).  Leaves the scores of the piece's LAST chunk staged: all of them for cnt <= 64.
__device__ __forceinline__ float piece_max(float *stage, const GatJob &job, uint32_t v, uint32_t p0, uint32_t cnt,
                                           uint32_t lane) {
  const uint32_t H = job.H, Hp = pow2_heads(H), h = lane & (Hp - 1u), g = lane / Hp, G = kWave / Hp;
  float m = -__builtin_inff();
  for (uint32_t c0 = 0; c0 < cnt; c0 += kWave) {
    const uint32_t n = cnt - c0 < (uint32_t)kWave ? cnt - c0 : (uint32_t)kWave;
    stage_sync();  // the reads of the chunk before are done
    stage_scores(stage, job, v, lane < n ? job.indices[p0 + c0 + lane] : 0u, lane < n, lane);
    stage_sync();
    if (h < H) {
      for (uint32_t e = g; e < n; e += G) m = fmaxf(m, stage[e * H + h]);
    }
  }
  for (uint32_t d = Hp; d < (uint32_t)kWave; d <<= 1) m = fmaxf(m, __shfl_xor(m, (int)d, kWave));
  return m;
}

// Lane l owns columns dbase + l + 64 q.  acc[q] and z[q] start at 0 and add, in CSR order, the products w feat and the
// weights w = exp(s - m_k[head of the column]) of the cnt (<= kCsrSplit) edges from position p0 on; mk = piece_max's
// result.  weights_staged: an earlier pass over other columns left this piece's weights staged, if it has at most 64.
// Otherwise a piece of cnt <= 64 finds its SCORES staged (piece_max) and longer pieces compute theirs again.  All lanes
// run the loops (the shuffles need them), loads are masked by act[q].  UN row loads are in flight together.
template <int P>
__device__ __forceinline__ void piece_sums(float (&acc)[P], float (&z)[P], const bool (&act)[P],
                                           const uint32_t (&head)[P], float *stage, const GatJob &job, uint32_t v,
                                           uint32_t dbase, uint32_t p0, uint32_t cnt, float mk, bool weights_staged,
                                           uint32_t lane) {
  constexpr uint32_t UN = 4;
  const uint32_t H = job.H;
  const bool staged = weights_staged && cnt <= (uint32_t)kWave;
#pragma unroll
  for (int q = 0; q < P; ++q) acc[q] = z[q] = 0.0f;
  for (uint32_t c0 = 0; c0 < cnt; c0 += kWave) {
    const uint32_t n = cnt - c0 < (uint32_t)kWave ? cnt - c0 : (uint32_t)kWave;
    const uint32_t my_src = lane < n ? job.indices[p0 + c0 + lane] : 0u;
    if (!staged) {  // wave-uniform
      stage_sync();  // the reads of the chunk before, or of piece_max, are done
      if (cnt > (uint32_t)kWave) stage_scores(stage, job, v, my_src, lane < n, lane);
      for (uint32_t h = 0; h < H; ++h) {  // every lane takes part in the shuffle
        const float mh = __shfl(mk, (int)h, kWave);
        if (lane < n) stage[lane * H + h] = expf(stage[lane * H + h] - mh);
      }
      stage_sync();
    }
    for (uint32_t i0 = 0; i0 < n; i0 += UN) {
      float f[UN][P], we[UN][P];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t i = i0 + u < n ? i0 + u : n - 1;  // clamp: the extra loads are discarded below
        const uint32_t sidx = __shfl(my_src, (int)i, kWave);
        const float *fp = job.feat + (size_t)sidx * job.feat_ld + dbase + lane;
        const float *wp = stage + i * H;
#pragma unroll
        for (int q = 0; q < P; ++q) {
          f[u][q] = act[q] ? fp[kWave * q] : 0.0f;
          we[u][q] = wp[head[q]];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (i0 + u >= n) break;  // wave-uniform
#pragma unroll
        for (int q = 0; q < P; ++q) {
          acc[q] += we[u][q] * f[u][q];
          z[q] += we[u][q];
        }
      }
    }
  }
}

// the columns of pass dbase a lane owns: in range?  which head (0 for a column out of range: a valid staging index)
template <int P>
__device__ __forceinline__ void set_columns(bool (&act)[P], uint32_t (&head)[P], const GatJob &job, uint32_t dbase,
                                            uint32_t lane) {
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const uint32_t c = dbase + lane + kWave * q;
    act[q] = c < job.dim;
    head[q] = act[q] ? c / job.F : 0u;
  }
}

// Row pass: wave (blockIdx.x, wave_id) owns output row i.  A row of more than kCsrSplit edges goes to the hub queue if
// the workspace has room for it (it always has when the caller's max_edges holds); otherwise its owner computes it
// here, piece by piece -- the same operations in the same order.
template <int P>
__global__ __launch_bounds__(kBlock) void csr_gat_rows_kernel(GatJob job, CsrWs ws, float *out, size_t num_rows,
                                                              uint32_t out_ld) {
  __shared__ float stage_all[kWavesPerBlock][kWave * kMaxHeads];
  const size_t i = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  if (i >= num_rows) return;  // wave-uniform
  float *stage = stage_all[wave_id()];
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t v = job_node(job, i);
  const uint32_t beg = job.indptr[v], len = job.indptr[v + 1] - beg;
  const uint32_t np = piece_count(len);
  if (np > 1 && ws.hub_cap && csr_queue_hub(ws, (uint32_t)i, np, lane)) return;  // wave-uniform
  float *op = out + i * out_ld;
  if (len == 0) {
    for (uint32_t c = lane; c < job.dim; c += kWave) op[c] = 0.0f;
    return;
  }
  // m = max_k m_k; for a row of one piece that is m_0, and its scores stay staged where it has at most 64 edges
  float m = -__builtin_inff();
  for (uint32_t k = 0; k < np; ++k) {
    const uint32_t done = k * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
    m = fmaxf(m, piece_max(stage, job, v, beg + done, cnt, lane));
  }
  for (uint32_t dbase = 0; dbase < job.dim; dbase += kWave * P) {  // one trip for dim <= 64 P
    bool act[P];
    uint32_t head[P];
    set_columns<P>(act, head, job, dbase, lane);
    float A[P] = {}, Z[P] = {};
    for (uint32_t k = 0; k < np; ++k) {
      const uint32_t done = k * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
      const float mk = np == 1 ? m : piece_max(stage, job, v, beg + done, cnt, lane);
      float acc[P], z[P];
      piece_sums<P>(acc, z, act, head, stage, job, v, dbase, beg + done, cnt, mk, np == 1 && dbase > 0, lane);
#pragma unroll
      for (int q = 0; q < P; ++q) {
        const float c = expf(__shfl(mk, (int)head[q], kWave) - __shfl(m, (int)head[q], kWave));
        Z[q] += c * z[q];
        A[q] += c * acc[q];
      }
    }
#pragma unroll
    for (int q = 0; q < P; ++q)
      if (act[q]) op[dbase + lane + kWave * q] = A[q] / Z[q];
  }
}

// Hub pass 1: the waves of the grid walk the piece descriptors the row pass wrote (their number is read from device
// memory) and leave every piece's (acc_k [dim] | z_k [H] | m_k [H]) in its partial row.
template <int P>
__global__ __launch_bounds__(kBlock) void csr_gat_hub_pieces_kernel(GatJob job, CsrWs ws) {
  __shared__ float stage_all[kWavesPerBlock][kWave * kMaxHeads];
  float *stage = stage_all[wave_id()];
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t handed = ws.counts[1], n = handed < ws.piece_cap ? handed : ws.piece_cap;
  const uint32_t stride = gridDim.x * kWavesPerBlock;
  const size_t width = (size_t)job.dim + 2 * job.H;
  for (uint32_t p = blockIdx.x * kWavesPerBlock + wave_id(); p < n; p += stride) {
    const uint2 d = ws.pieces[p];
    if (d.x == kNoRow) continue;  // wave-uniform
    const uint32_t v = job_node(job, d.x);
    const uint32_t beg = job.indptr[v], len = job.indptr[v + 1] - beg;
    const uint32_t done = d.y * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
    float *pp = ws.partial + (size_t)p * width;
    const float mk = piece_max(stage, job, v, beg + done, cnt, lane);
    if (lane < job.H) pp[job.dim + job.H + lane] = mk;
    for (uint32_t dbase = 0; dbase < job.dim; dbase += kWave * P) {
      bool act[P];
      uint32_t head[P];
      set_columns<P>(act, head, job, dbase, lane);
      float acc[P], z[P];
      piece_sums<P>(acc, z, act, head, stage, job, v, dbase, beg + done, cnt, mk, dbase > 0, lane);
#pragma unroll
      for (int q = 0; q < P; ++q) {
        const uint32_t c = dbase + lane + kWave * q;
        if (!act[q]) continue;
        pp[c] = acc[q];
        if (c == head[q] * job.F) pp[job.dim + head[q]] = z[q];  // the head's first column stores its sum of weights
      }
    }
  }
}

// Hub pass 2: one wave per (queued hub, 64 columns) combines the hub's partial rows IN PIECE ORDER, starting at 0 --
// the operations the row pass makes for a row it computes itself -- and stores the output row.
__global__ __launch_bounds__(kBlock) void csr_gat_hub_combine_kernel(GatJob job, CsrWs ws, float *out, uint32_t out_ld) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t queued = ws.counts[0], nh = queued < ws.hub_cap ? queued : ws.hub_cap;
  const uint32_t chunks = (job.dim + kWave - 1) / kWave;
  const size_t items = (size_t)nh * chunks, stride = (size_t)gridDim.x * kWavesPerBlock;
  const size_t width = (size_t)job.dim + 2 * job.H;
  for (size_t it = (size_t)blockIdx.x * kWavesPerBlock + wave_id(); it < items; it += stride) {
    const uint2 hub = ws.hubs[it / chunks];
    if (hub.x == kNoRow) continue;  // wave-uniform
    const uint32_t c = (uint32_t)(it % chunks) * kWave + lane;
    if (c >= job.dim) continue;
    const uint32_t v = job_node(job, hub.x);
    const uint32_t np = piece_count(job.indptr[v + 1] - job.indptr[v]);
    const float *pp = ws.partial + (size_t)hub.y * width;
    const uint32_t h = c / job.F;
    float m = -__builtin_inff();
    for (uint32_t k = 0; k < np; ++k) m = fmaxf(m, pp[k * width + job.dim + job.H + h]);
    float A = 0.0f, Z = 0.0f;
    for (uint32_t k = 0; k < np; ++k) {
      const float *pk = pp + k * width;
      const float ck = expf(pk[job.dim + job.H + h] - m);
      Z += ck * pk[job.dim + h];
      A += ck * pk[c];
    }
    out[(size_t)hub.x * out_ld + c] = A / Z;
  }
}

// the instantiation by dim (columns per lane and pass); the hub passes where a hub is possible
void launch_csr_gat(const GatJob &job, const CsrWs &ws, float *out, size_t num_rows, uint32_t out_ld,
                    hipStream_t stream) {
  static constexpr decltype(&csr_gat_rows_kernel<1>) rows[3] = {csr_gat_rows_kernel<1>, csr_gat_rows_kernel<2>,
                                                                csr_gat_rows_kernel<4>};
  static constexpr decltype(&csr_gat_hub_pieces_kernel<1>) pieces[3] = {
      csr_gat_hub_pieces_kernel<1>, csr_gat_hub_pieces_kernel<2>, csr_gat_hub_pieces_kernel<4>};
  const int which = job.dim <= (uint32_t)kWave ? 0 : (job.dim <= 2u * kWave ? 1 : 2);
  hipLaunchKernelGGL(rows[which], dim3(div_up(num_rows, (size_t)kWavesPerBlock)), dim3(kBlock), 0, stream, job, ws, out,
                     num_rows, out_ld);
  if (!ws.hub_cap) return;
  const size_t pg = div_up((size_t)ws.piece_cap, (size_t)kWavesPerBlock);
  hipLaunchKernelGGL(pieces[which], dim3(pg < kHubGridBlocks ? pg : kHubGridBlocks), dim3(kBlock), 0, stream, job, ws);
  const size_t cg = div_up((size_t)ws.hub_cap * div_up((size_t)job.dim, (size_t)kWave), (size_t)kWavesPerBlock);
  hipLaunchKernelGGL(csr_gat_hub_combine_kernel, dim3(cg < kHubGridBlocks ? cg : kHubGridBlocks), dim3(kBlock), 0,
                     stream, job, ws, out, out_ld);
}

// floats of a partial row: acc_k | z_k | m_k
inline size_t gat_partial_width(size_t num_head, size_t num_feat) { return num_head * num_feat + 2 * num_head; }

}  // namespace
}  // namespace fgnn

extern "C" size_t fgnn_csr_gat_max_heads(void) { return fgnn::kMaxHeads; }

extern "C" size_t fgnn_csr_gat_workspace_bytes(size_t num_rows, size_t max_edges, size_t num_head, size_t num_feat) {
  return fgnn::csr_ws_layout(num_rows, max_edges, fgnn::gat_partial_width(num_head, num_feat)).bytes;
}

extern "C" int fgnn_csr_gat_attention(const uint32_t *indptr, const uint32_t *indices, const uint32_t *nodes,
                                      size_t first, size_t num_rows, size_t max_edges, const float *el, const float *er,
                                      const float *feat, size_t feat_ld, size_t num_head, size_t num_feat,
                                      float negative_slope, float *out, size_t out_ld, void *ws, size_t ws_bytes,
                                      void *stream) {
  using namespace fgnn;
  if (num_rows == 0) return FGNN_OK;
  if (!indptr || !indices || !el || !er || !feat || !out || num_head == 0 || num_feat == 0 || num_head > kMaxHeads)
    return FGNN_EINVAL;
  if (!float_aligned(indptr) || !float_aligned(indices) || !float_aligned(nodes) || !float_aligned(el) ||
      !float_aligned(er) || !float_aligned(feat) || !float_aligned(out))
    return FGNN_EINVAL;
  if (!fits_u32(num_feat) || !fits_u32(num_head * num_feat)) return FGNN_EINVAL;
  const size_t dim = num_head * num_feat;
  if (feat_ld < dim || !fits_u32(feat_ld) || out_ld < dim || !fits_u32(out_ld)) return FGNN_EINVAL;
  if (!csr_rows_in_range(nodes != nullptr, first, num_rows, max_edges)) return FGNN_EINVAL;
  const CsrWsLayout l = csr_ws_layout(num_rows, max_edges, gat_partial_width(num_head, num_feat));
  if (!csr_ws_ok(l, ws, ws_bytes)) return FGNN_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CsrWs w = csr_ws_view(l, ws);
  if (l.bytes) FGNN_HIP_CHECK(hipMemsetAsync(w.counts, 0, 16, s));
  const GatJob job{indptr, indices, nodes, el, er, feat, (uint32_t)first, (uint32_t)num_head, (uint32_t)num_feat,
                   (uint32_t)dim, (uint32_t)feat_ld, negative_slope};
  launch_csr_gat(job, w, out, num_rows, (uint32_t)out_ld, s);
  return launch_status(__func__);
}
