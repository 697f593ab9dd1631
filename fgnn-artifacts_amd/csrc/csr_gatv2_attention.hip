// csr_gatv2_attention.hip -- a GATv2 layer's attention aggregation over whole CSR rows: the message-passing step of exact
// layer-wise GATv2 inference on the full graph (examples/inference.py: gatv2_layerwise_inference).  H heads of F
// features, D = H F; for output row i, v = nodes ? nodes[i] : first + i, over p in [indptr[v], indptr[v + 1]):
//     s[p,h] = sum_f attn[h,f] leaky_relu(fs[indices[p],h,f] + fd[v,h,f])     a[p,h] = softmax of s[.,h] over the row
//     out[i,h,:] = sum_p a[p,h] fs[indices[p],h,:]
// gatv2_attention.hip serves sampled COO blocks and training (a destination per edge, 2 E H floats of scratch, a
// pre-filled output, float atomics).  csr_gat_attention.hip's kernel does not fit either: GAT's score is a scalar per
// (edge, head) read from el and er, cheap enough to compute twice (a max pass, then a sum pass).  Here the score is a
// reduction over the WHOLE neighbour row behind a nonlinearity: a max pass would read every fs row twice.  So this
// kernel makes ONE pass with an online softmax in fixed blocks, and every fs element is read once.
// Contract (csr_gat_attention.hip's): out is overwritten, a row without a neighbour writes zeros, fd is indexed by NODE
// id and may be fs itself, no dropout, no alpha output, no atomic on a float, fp32 only.
// Who owns what.  ONE wave owns an output row.  The columns are walked in trips of W = floor(64 P / F) F columns (P = 1,
// 2, 4 slots per lane by D), so that a trip holds whole heads: the softmax of a head never leaves its trip, and a trip
// walks the row's edges once.  Lane l owns columns tb + l + 64 q of the trip at tb; its attn and fd[v] slots stay in
// registers for the whole row.  Neighbour ids are loaded 64 at a time, coalesced, and broadcast by shuffle; the fs rows
// of a block of B = kBlockEdges edges are in flight together.
// The order of the operations is fixed by the row alone.  A row is cut into pieces of kCsrSplit edges.  A piece is
// walked in CSR order in blocks of B edges (the last one shorter), from m = -inf, z = 0, acc = 0; per block and head
//     m' = max(m, s_0, ..)   c = exp(m - m')   w_j = exp(s_j - m')
//     acc = c acc + w_0 f_0 + w_1 f_1 ..        z = c z + w_0 + w_1 ..        m = m'      (left to right)
// which leaves the piece's (acc_k, z_k, m_k); exp(-inf) = 0 starts the first block, and a row of one edge ends with acc
// = 0 * 0 + 1 * f, z = 1.  The row combines its pieces exactly as csr_gat_attention.hip does: m = max_k m_k, c_k =
// exp(m_k - m), Z = 0 + c_k z_k .., A = 0 + c_k acc_k .., out = A / Z.  Who computes a piece does not enter: rows of one
// piece and rows the workspace has no room for are computed by their owner wave (which, for a row of several pieces,
// walks it twice: the m_k first, since c_k needs m -- a path only an understated max_edges takes), longer rows are
// queued by the row pass (csr_queue.h), their pieces left as (acc_k | z_k | m_k) in partial rows by a second launch and
// combined by a third.  Three stream-ordered launches (one where no row can be a hub), one 16-byte memset, no host
// synchronisation.
// The score's reduction over F, the sum order being part of the definition (a kernel template parameter, by shape):
//   kGroups  F a power of two <= 64: a head is an aligned group of F lanes in a slot, reduced by xor shuffles
//            (distances F/2 .. 1); every lane of the group ends with the same bits (a + b = b + a at every level)
//   kWhole   a trip holds ONE head (H = 1, or F > 32 P): the lane's slots are summed in slot order, then xor shuffles
//            over the whole wave (32 .. 1); columns out of range contribute 0.  The output layers: 1 x 47, 1 x 172
//   kStaged  every other shape (3 x 7, 4 x 33): the block's products go to a per-wave LDS stage [B][64 P], lane j sums
//            the F products of (edge j / Ht, head j % Ht) in column order (Ht = heads of the trip), leaves the score in
//            [B][Ht] behind it, and every lane reads the scores of its slots' heads back.  Only the owning wave touches
//            its stage: no barrier, a wavefront-scope fence orders the compiler (csr_gat_attention.hip's stage_sync).
//            Dynamic LDS, none for the two other modes.
// All lanes of a head hold the same m, z and weights, computed from the same bits.  No register array is indexed
// dynamically.  Matrix instructions do not fit: every product sits behind a per-element nonlinearity on an indexed pair
// of rows.  F <= kMaxFeats = 256 (fgnn_csr_gatv2_max_feats; a trip of 4 slots holds a head); any H.
// Index widths as in csr_aggregate.hip: edge positions and node ids are uint32_t, every address into fs, fd, out and
// the partial rows is formed in size_t.
#include "csr_queue.h"

namespace fgnn {
namespace {

constexpr uint32_t kBlockEdges = 4;   // B: edges of an online-softmax block = fs rows in flight
constexpr uint32_t kMaxFeats = 256;   // a head fits the widest trip (4 slots per lane)

enum ScoreMode : int { kGroups = 0, kWhole = 1, kStaged = 2 };

// The graph, the rows asked for and the layer's projections: what all three kernels read.
struct Gatv2Job {
  const uint32_t *indptr, *indices, *nodes;
  const float *fs, *fd, *attn;
  uint32_t first, H, F, dim, fs_ld, fd_ld;
  uint32_t trip;  // columns of a trip: whole heads, at most 64 P
  float slope;
};
__device__ __forceinline__ uint32_t job_node(const Gatv2Job &j, size_t i) {
  return j.nodes ? j.nodes[i] : j.first + (uint32_t)i;
}

// orders the wave's own LDS writes and reads (different lanes, same wave) for the compiler; the hardware runs a wave's
// LDS operations in order
__device__ __forceinline__ void stage_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// exp of the block loop, B + 1 per slot and block in every lane: the hardware's exp2 of x log2(e), two instructions
// where expf is twenty.  Arguments are <= 0; exp(0) = 1 and exp(-inf) = 0 exactly; the relative error grows with |x|
// (about 2^-23 |x|), where the weight itself shrinks as e^x.  The few exponentials per ROW (c_k) stay expf.
__device__ __forceinline__ float fast_exp(float x) { return __expf(x); }

// floats of a wave's stage (kStaged): the block's products, then its scores
inline size_t stage_floats(int P, size_t trip, size_t F) { return kBlockEdges * ((size_t)kWave * P + trip / F); }

// What a lane keeps of the trip at column tb for the whole row: which of its slots are in range, their head within the
// trip (0 out of range: a valid stage index), their attn and fd[v] values (0 out of range: the product is 0).
template <int P>
struct Columns {
  bool act[P];
  uint32_t hl[P];
  float av[P], fdv[P];
};
template <int P>
__device__ __forceinline__ void set_columns(Columns<P> &c, const Gatv2Job &job, uint32_t v, uint32_t tb, uint32_t wt,
                                            uint32_t lane) {
  const float *dp = job.fd + (size_t)v * job.fd_ld + tb + lane;
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const uint32_t cl = lane + kWave * q;
    c.act[q] = cl < wt;
    c.hl[q] = c.act[q] ? cl / job.F : 0u;
    c.av[q] = c.act[q] ? job.attn[tb + cl] : 0.0f;
    c.fdv[q] = c.act[q] ? dp[kWave * q] : 0.0f;
  }
}

// s[u][q] <- the score of edge u of the block for the head of slot q, from the fs values f[u][q] (0 out of range)
template <int P, int MODE>
__device__ __forceinline__ void block_scores(float (&s)[kBlockEdges][P], const float (&f)[kBlockEdges][P],
                                             const Columns<P> &c, const Gatv2Job &job, float *stage, uint32_t wt,
                                             uint32_t lane) {
#pragma unroll
  for (uint32_t u = 0; u < kBlockEdges; ++u) {
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const float x = f[u][q] + c.fdv[q];
      s[u][q] = c.av[q] * (x > 0.0f ? x : job.slope * x);
    }
  }
  if (MODE == kGroups) {
    // distances F/2 .. 1 of the six a wave has; the partner's byte address per distance is the lane's alone and is
    // hoisted out of the edge loops by the compiler, which leaves one ds_bpermute and one add per value and level
#pragma unroll
    for (uint32_t d = kWave / 2; d > 0; d >>= 1) {
      if (d >= job.F) continue;  // wave-uniform
      const int partner = (int)((lane ^ d) << 2);
#pragma unroll
      for (uint32_t u = 0; u < kBlockEdges; ++u) {
#pragma unroll
        for (int q = 0; q < P; ++q)
          s[u][q] += __int_as_float(__builtin_amdgcn_ds_bpermute(partner, __float_as_int(s[u][q])));
      }
    }
  } else if (MODE == kWhole) {
#pragma unroll
    for (uint32_t u = 0; u < kBlockEdges; ++u) {
      float t = s[u][0];
#pragma unroll
      for (int q = 1; q < P; ++q) t += s[u][q];
#pragma unroll
      for (int d = kWave / 2; d > 0; d >>= 1) t += __shfl_xor(t, d, kWave);
#pragma unroll
      for (int q = 0; q < P; ++q) s[u][q] = t;
    }
  } else {
    constexpr uint32_t kRow = kWave * P;
    const uint32_t F = job.F, ht = wt / F, ld = job.trip / F;  // heads of this trip; row length of the score stage
    float *sc = stage + kBlockEdges * kRow;
    stage_sync();  // the reads of the block before are done
#pragma unroll
    for (uint32_t u = 0; u < kBlockEdges; ++u) {
#pragma unroll
      for (int q = 0; q < P; ++q)
        if (c.act[q]) stage[u * kRow + lane + kWave * q] = s[u][q];
    }
    stage_sync();
    for (uint32_t j = lane; j < kBlockEdges * ht; j += kWave) {
      const uint32_t u = j / ht, h = j - u * ht;
      const float *pp = stage + u * kRow + h * F;
      float t = 0.0f;
      for (uint32_t k = 0; k < F; ++k) t += pp[k];
      sc[u * ld + h] = t;
    }
    stage_sync();
#pragma unroll
    for (uint32_t u = 0; u < kBlockEdges; ++u) {
#pragma unroll
      for (int q = 0; q < P; ++q) s[u][q] = sc[u * ld + c.hl[q]];
    }
  }
}

// One piece: the cnt (1 .. kCsrSplit) edges from position p0 on, in blocks of kBlockEdges, for the trip at column tb.
// Leaves (acc_k, z_k, m_k) per slot; m and z are the same in every lane of a head.  All lanes run every loop (the
// shuffles need them); loads are masked by act[q].
template <int P, int MODE>
__device__ __forceinline__ void piece_walk(float (&m)[P], float (&z)[P], float (&acc)[P], const Columns<P> &c,
                                           const Gatv2Job &job, float *stage, uint32_t tb, uint32_t wt, uint32_t p0,
                                           uint32_t cnt, uint32_t lane) {
#pragma unroll
  for (int q = 0; q < P; ++q) {
    m[q] = -__builtin_inff();
    z[q] = acc[q] = 0.0f;
  }
  for (uint32_t c0 = 0; c0 < cnt; c0 += kWave) {
    const uint32_t n = cnt - c0 < (uint32_t)kWave ? cnt - c0 : (uint32_t)kWave;
    const uint32_t my_src = lane < n ? job.indices[p0 + c0 + lane] : 0u;
    for (uint32_t i0 = 0; i0 < n; i0 += kBlockEdges) {
      const uint32_t nb = n - i0;  // live edges of the block (wave-uniform); kBlockEdges or more: all
      float f[kBlockEdges][P], s[kBlockEdges][P];
#pragma unroll
      for (uint32_t u = 0; u < kBlockEdges; ++u) {
        const uint32_t i = u < nb ? i0 + u : n - 1;  // clamp: the extra rows are discarded below
        const uint32_t sidx = __shfl(my_src, (int)i, kWave);
        const float *fp = job.fs + (size_t)sidx * job.fs_ld + tb + lane;
#pragma unroll
        for (int q = 0; q < P; ++q) f[u][q] = c.act[q] ? fp[kWave * q] : 0.0f;
      }
      block_scores<P, MODE>(s, f, c, job, stage, wt, lane);
#pragma unroll
      for (int q = 0; q < P; ++q) {
        float mx = m[q];
#pragma unroll
        for (uint32_t u = 0; u < kBlockEdges; ++u)
          if (u < nb) mx = fmaxf(mx, s[u][q]);
        const float cf = fast_exp(m[q] - mx);  // the first block: exp(-inf) = 0
        float a = cf * acc[q], zz = cf * z[q];
#pragma unroll
        for (uint32_t u = 0; u < kBlockEdges; ++u) {
          if (u < nb) {
            const float w = fast_exp(s[u][q] - mx);
            a += w * f[u][q];
            zz += w;
          }
        }
        m[q] = mx;
        acc[q] = a;
        z[q] = zz;
      }
    }
  }
}

// Row pass: wave (blockIdx.x, wave_id) owns output row i.  A row of more than kCsrSplit edges goes to the hub queue if
// the workspace has room for it (it always has when the caller's max_edges holds); otherwise its owner computes it
// here -- pass 0 for m = max_k m_k, pass 1 for the sums: the same operations in the same order as the hub passes.
template <int P, int MODE>
__global__ __launch_bounds__(kBlock) void csr_gatv2_rows_kernel(Gatv2Job job, CsrWs ws, float *out, size_t num_rows,
                                                                uint32_t out_ld, uint32_t stage_ld) {
  extern __shared__ float stage_all[];
  const size_t i = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  if (i >= num_rows) return;  // wave-uniform
  float *stage = stage_all + (size_t)wave_id() * stage_ld;
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
  for (uint32_t tb = 0; tb < job.dim; tb += job.trip) {  // one trip where all heads fit 64 P columns
    const uint32_t wt = job.dim - tb < job.trip ? job.dim - tb : job.trip;
    Columns<P> col;
    set_columns<P>(col, job, v, tb, wt, lane);
    float mrow[P], A[P], Z[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
      mrow[q] = -__builtin_inff();
      A[q] = Z[q] = 0.0f;
    }
    for (uint32_t pass = np > 1 ? 0u : 1u; pass < 2u; ++pass) {
      for (uint32_t k = 0; k < np; ++k) {
        const uint32_t done = k * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
        float mk[P], zk[P], acck[P];
        piece_walk<P, MODE>(mk, zk, acck, col, job, stage, tb, wt, beg + done, cnt, lane);
#pragma unroll
        for (int q = 0; q < P; ++q) {
          if (pass == 0u || np == 1u) mrow[q] = fmaxf(mrow[q], mk[q]);
          if (pass == 1u) {
            const float ck = expf(mk[q] - mrow[q]);
            Z[q] += ck * zk[q];
            A[q] += ck * acck[q];
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < P; ++q)
      if (col.act[q]) op[tb + lane + kWave * q] = A[q] / Z[q];
  }
}

// Hub pass 1: the waves of the grid walk the piece descriptors the row pass wrote (their number is read from device
// memory) and leave every piece's (acc_k [dim] | z_k [H] | m_k [H]) in its partial row.
template <int P, int MODE>
__global__ __launch_bounds__(kBlock) void csr_gatv2_hub_pieces_kernel(Gatv2Job job, CsrWs ws, uint32_t stage_ld) {
  extern __shared__ float stage_all[];
  float *stage = stage_all + (size_t)wave_id() * stage_ld;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t handed = ws.counts[1], n = handed < ws.piece_cap ? handed : ws.piece_cap;
  const uint32_t stride = gridDim.x * kWavesPerBlock;
  const size_t width = (size_t)job.dim + 2 * (size_t)job.H;
  for (uint32_t p = blockIdx.x * kWavesPerBlock + wave_id(); p < n; p += stride) {
    const uint2 d = ws.pieces[p];
    if (d.x == kNoRow) continue;  // wave-uniform
    const uint32_t v = job_node(job, d.x);
    const uint32_t beg = job.indptr[v], len = job.indptr[v + 1] - beg;
    const uint32_t done = d.y * kCsrSplit, cnt = len - done < kCsrSplit ? len - done : kCsrSplit;
    float *pp = ws.partial + (size_t)p * width;
    for (uint32_t tb = 0; tb < job.dim; tb += job.trip) {
      const uint32_t wt = job.dim - tb < job.trip ? job.dim - tb : job.trip;
      Columns<P> col;
      set_columns<P>(col, job, v, tb, wt, lane);
      float mk[P], zk[P], acck[P];
      piece_walk<P, MODE>(mk, zk, acck, col, job, stage, tb, wt, beg + done, cnt, lane);
#pragma unroll
      for (int q = 0; q < P; ++q) {
        if (!col.act[q]) continue;
        const uint32_t c = tb + lane + kWave * q, h = c / job.F;
        pp[c] = acck[q];
        if (c == h * job.F) {  // the head's first column stores its sum of weights and its max
          pp[job.dim + h] = zk[q];
          pp[(size_t)job.dim + job.H + h] = mk[q];
        }
      }
    }
  }
}

// Hub pass 2: one wave per (queued hub, 64 columns) combines the hub's partial rows IN PIECE ORDER, starting at 0 --
// the operations the row pass makes for a row it computes itself -- and stores the output row.  (The form of
// csr_gat_attention.hip's combine; a copy, so that file compiles to what it was.)
__global__ __launch_bounds__(kBlock) void csr_gatv2_hub_combine_kernel(Gatv2Job job, CsrWs ws, float *out,
                                                                       uint32_t out_ld) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t queued = ws.counts[0], nh = queued < ws.hub_cap ? queued : ws.hub_cap;
  const uint32_t chunks = (job.dim + kWave - 1) / kWave;
  const size_t items = (size_t)nh * chunks, stride = (size_t)gridDim.x * kWavesPerBlock;
  const size_t width = (size_t)job.dim + 2 * (size_t)job.H;
  for (size_t it = (size_t)blockIdx.x * kWavesPerBlock + wave_id(); it < items; it += stride) {
    const uint2 hub = ws.hubs[it / chunks];
    if (hub.x == kNoRow) continue;  // wave-uniform
    const uint32_t c = (uint32_t)(it % chunks) * kWave + lane;
    if (c >= job.dim) continue;
    const uint32_t v = job_node(job, hub.x);
    const uint32_t np = piece_count(job.indptr[v + 1] - job.indptr[v]);
    const float *pp = ws.partial + (size_t)hub.y * width;
    const size_t zat = (size_t)job.dim + c / job.F, mat = zat + job.H;
    float m = -__builtin_inff();
    for (uint32_t k = 0; k < np; ++k) m = fmaxf(m, pp[k * width + mat]);
    float A = 0.0f, Z = 0.0f;
    for (uint32_t k = 0; k < np; ++k) {
      const float *pk = pp + k * width;
      const float ck = expf(pk[mat] - m);
      Z += ck * pk[zat];
      A += ck * pk[c];
    }
    out[(size_t)hub.x * out_ld + c] = A / Z;
  }
}

// slots per lane by D; a head always fits: F <= D, and F <= kMaxFeats = 256 where D is larger
inline int gatv2_slots(size_t dim) { return dim <= (size_t)kWave ? 1 : (dim <= 2u * kWave ? 2 : 4); }
// how the products of a head are summed
inline int gatv2_mode(size_t H, size_t F, int P) {
  if (F <= (size_t)kWave && (F & (F - 1)) == 0) return kGroups;
  return H == 1 || (size_t)kWave * P / F == 1 ? kWhole : kStaged;
}

template <int MODE>
void launch_csr_gatv2_mode(int which, const Gatv2Job &job, const CsrWs &ws, float *out, size_t num_rows,
                           uint32_t out_ld, hipStream_t stream) {
  static constexpr decltype(&csr_gatv2_rows_kernel<1, MODE>) rows[3] = {
      csr_gatv2_rows_kernel<1, MODE>, csr_gatv2_rows_kernel<2, MODE>, csr_gatv2_rows_kernel<4, MODE>};
  static constexpr decltype(&csr_gatv2_hub_pieces_kernel<1, MODE>) pieces[3] = {
      csr_gatv2_hub_pieces_kernel<1, MODE>, csr_gatv2_hub_pieces_kernel<2, MODE>, csr_gatv2_hub_pieces_kernel<4, MODE>};
  const size_t stage_ld = MODE == kStaged ? stage_floats(1 << which, job.trip, job.F) : 0;
  const size_t lds = kWavesPerBlock * stage_ld * sizeof(float);  // 21.4 KiB at most (P = 4, F = 3)
  hipLaunchKernelGGL(rows[which], dim3(div_up(num_rows, (size_t)kWavesPerBlock)), dim3(kBlock), lds, stream, job, ws,
                     out, num_rows, out_ld, (uint32_t)stage_ld);
  if (!ws.hub_cap) return;
  const size_t pg = div_up((size_t)ws.piece_cap, (size_t)kWavesPerBlock);
  hipLaunchKernelGGL(pieces[which], dim3(pg < kHubGridBlocks ? pg : kHubGridBlocks), dim3(kBlock), lds, stream, job, ws,
                     (uint32_t)stage_ld);
  const size_t cg = div_up((size_t)ws.hub_cap * div_up((size_t)job.dim, (size_t)kWave), (size_t)kWavesPerBlock);
  hipLaunchKernelGGL(csr_gatv2_hub_combine_kernel, dim3(cg < kHubGridBlocks ? cg : kHubGridBlocks), dim3(kBlock), 0,
                     stream, job, ws, out, out_ld);
}

// floats of a partial row: acc_k | z_k | m_k
inline size_t gatv2_partial_width(size_t num_head, size_t num_feat) { return num_head * num_feat + 2 * num_head; }
inline bool gatv2_shape_ok(size_t num_head, size_t num_feat) {
  return num_head != 0 && num_feat != 0 && num_feat <= kMaxFeats && fits_u32(num_head) &&
         fits_u32(gatv2_partial_width(num_head, num_feat));
}

}  // namespace
}  // namespace fgnn

extern "C" size_t fgnn_csr_gatv2_max_feats(void) { return fgnn::kMaxFeats; }
extern "C" size_t fgnn_csr_gatv2_block_edges(void) { return fgnn::kBlockEdges; }

extern "C" size_t fgnn_csr_gatv2_workspace_bytes(size_t num_rows, size_t max_edges, size_t num_head, size_t num_feat) {
  if (!fgnn::gatv2_shape_ok(num_head, num_feat)) return 0;
  return fgnn::csr_ws_layout(num_rows, max_edges, fgnn::gatv2_partial_width(num_head, num_feat)).bytes;
}

extern "C" int fgnn_csr_gatv2_attention(const uint32_t *indptr, const uint32_t *indices, const uint32_t *nodes,
                                        size_t first, size_t num_rows, size_t max_edges, const float *fs, size_t fs_ld,
                                        const float *fd, size_t fd_ld, const float *attn, size_t num_head,
                                        size_t num_feat, float negative_slope, float *out, size_t out_ld, void *ws,
                                        size_t ws_bytes, void *stream) {
  using namespace fgnn;
  if (num_rows == 0) return FGNN_OK;
  if (!indptr || !indices || !fs || !fd || !attn || !out || !gatv2_shape_ok(num_head, num_feat)) return FGNN_EINVAL;
  if (!float_aligned(indptr) || !float_aligned(indices) || !float_aligned(nodes) || !float_aligned(fs) ||
      !float_aligned(fd) || !float_aligned(attn) || !float_aligned(out))
    return FGNN_EINVAL;
  const size_t dim = num_head * num_feat;
  if (fs_ld < dim || !fits_u32(fs_ld) || fd_ld < dim || !fits_u32(fd_ld) || out_ld < dim || !fits_u32(out_ld))
    return FGNN_EINVAL;
  if (!csr_rows_in_range(nodes != nullptr, first, num_rows, max_edges)) return FGNN_EINVAL;
  const CsrWsLayout l = csr_ws_layout(num_rows, max_edges, gatv2_partial_width(num_head, num_feat));
  if (!csr_ws_ok(l, ws, ws_bytes)) return FGNN_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CsrWs w = csr_ws_view(l, ws);
  if (l.bytes) FGNN_HIP_CHECK(hipMemsetAsync(w.counts, 0, 16, s));
  const int P = gatv2_slots(dim), which = P == 1 ? 0 : (P == 2 ? 1 : 2);
  const size_t trip = (size_t)kWave * P / num_feat * num_feat;
  const Gatv2Job job{indptr, indices, nodes, fs, fd, attn, (uint32_t)first, (uint32_t)num_head, (uint32_t)num_feat,
                     (uint32_t)dim, (uint32_t)fs_ld, (uint32_t)fd_ld, (uint32_t)trip, negative_slope};
  switch (gatv2_mode(num_head, num_feat, P)) {
    case kGroups: launch_csr_gatv2_mode<kGroups>(which, job, w, out, num_rows, (uint32_t)out_ld, s); break;
    case kWhole: launch_csr_gatv2_mode<kWhole>(which, job, w, out, num_rows, (uint32_t)out_ld, s); break;
    default: launch_csr_gatv2_mode<kStaged>(which, job, w, out, num_rows, (uint32_t)out_ld, s);
  }
  return launch_status(__func__);
}
