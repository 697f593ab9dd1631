// sample_khop_shared.hip -- fixed-fanout neighbour sampling with ONE random key per NODE (sequential Poisson sampling,
// the fixed-fanout form of LABOR: Balin & Catalyurek, "Layer-Neighbor Sampling").  Not a sampler of the reference.
//
// Every node t gets one 32-bit word per (batch, layer): w(t) = pick_word(philox_block(seed, batch_key, tag, t >> 2, 0),
// t & 3).  A seed with row indices[off .. off+len) gives position j the key (w(t_j) << 32) | j and keeps the `fanout`
// positions with the smallest keys, emitted in CSR order; rows of at most `fanout` entries are taken whole.  The words are
// i.i.d. uniform, so a seed's sample is a uniform k-subset like khop0's; seeds whose rows overlap prefer the SAME
// neighbours, which is the point: fewer distinct nodes enter the batch.  The result is a pure function of the inputs --
// it does not depend on how the work below is split.
//
// MI355X design.  The number of edges of a seed, min(len, fanout), is known from indptr alone: a workgroup (a tile of S
// seeds, 4 waves) publishes its edge count at once and has its output offset from the cross-workgroup prefix
// (fgnn_device.h) before it looks at a row, so rows are selected and written in one go.  (Frontiers of more than
// kSinglePassMaxTiles tiles, and the stateless entry point, which owns no descriptors: count -> scan -> emit.)
// Unlike khop2 every element of a row is read and pays a Philox block: node ids of a row are scattered, so the four
// words of a block rarely serve more than one element, and lanes run the ten rounds in lockstep anyway.  What the
// kernel saves is everything after that -- the word of an element is computed ONCE and kept where the selection runs:
//   * len <= fanout: a wave copies the row.
//   * fanout < len <= kWaveRow (1024): a wave owns the row.  Lane l holds elements l, l + 64, ... -- up to 16 words and
//     16 node ids in registers.  The fanout-th smallest word is found bit by bit from the top: one compare per held word,
//     the count of candidates whose bit is 0 is a ballot + scalar popcount (no LDS, no shuffles, 32 steps whatever the
//     fanout).  Equal words (a row that repeats a node id) are resolved by position; the row is then emitted by ballot
//     compaction, which is CSR order.  1024 = 16 registers per lane for the words and 16 for the ids: twice that spills.
//     The first 64 elements of a wave's NEXT row are loaded before the current row is selected.
//   * kWaveRow < len <= kBlockRow (8192): the workgroup owns the row: words in LDS (32 KiB, the most that still leaves
//     four workgroups per CU), the threshold by four passes over an 8-bit LDS histogram, ordered emit by block ranks.
//   * len > kBlockRow (hub rows; R-MAT rows reach 10^5..10^6 entries and sit in nearly every frontier): listed by a scan
//     before the sampler runs, cut into pieces of kBlockRow entries, and ALL workgroups of the chip reduce a piece each
//     to its `fanout` smallest (word, position) pairs -- the row's winners are among them.  The owner then selects among
//     pieces * fanout candidates streamed from the pool (a 10^6 row at fanout 64: 7808 pairs) instead of walking the
//     row.  A hub that finds no room in the pool (kMaxHubs = 16384 rows, kHubPool = 4 M pairs: a layer-0 frontier of the
//     papers100M-shaped graph lists thousands of hubs) stays with its owner, which streams the row itself and recomputes
//     the words in every pass: slow, the same result.
// Integer selection work throughout: no float atomics, no matrix instructions.
#include "fgnn_device.h"

namespace fgnn {
namespace {

constexpr uint32_t kMaxFanout = 64;    // the reference's configurations use <= 25
constexpr uint32_t kWaveRow = 1024;
constexpr uint32_t kBlockRow = 8192;
constexpr int kRegs = kWaveRow / kWave;     // words (and ids) a lane holds of a wave-owned row
constexpr uint32_t kMaxHubs = 16384;        // a layer-0 frontier of the papers100M-shaped R-MAT graph holds thousands
constexpr uint32_t kHubPool = 1u << 22;     // (word, position) pairs of all hubs' candidates: 32 MiB, + 16 MiB piece map

__device__ __forceinline__ uint32_t node_word(uint64_t seed, uint64_t batch_key, uint32_t tag, uint32_t t) {
  return pick_word(philox_block(seed, batch_key, tag, t >> 2, 0), t & 3u);
}

struct HubWs {
  uint32_t *of_seed;            // [cap] hub index of seed i, or FGNN_EMPTY_KEY
  uint32_t *count;              // [1] hubs claimed (may exceed kMaxHubs: the surplus stays with the owner)
  uint32_t *end;                // [1] end of the last claim that found room: pairs [0, *end) of the pool are in use
  unsigned long long *used;     // [1] pool pairs claimed, with or without room
  uint32_t *list;               // [kMaxHubs][4] row offset, row length, first pair in the pool, pieces (0: no room)
  uint32_t *cand_w, *cand_j;    // [kHubPool] candidates: word, position in the row; per piece in position order
  uint32_t *piece_hub;          // [kHubPool] hub of the piece whose candidates start at pair p * F
};

struct Threshold { uint32_t w, j; };  // an element is kept iff (word, position) <= (w, j)

// ---- the workgroup's selection: kBlock threads, M items, word_at(i) / pos_at(i) with pos ascending in i ---------------
struct BlockSelLds {
  uint32_t hist[256];
  uint32_t scan[kWavesPerBlock];
  uint32_t pick[2];
};

template <typename WordAt, typename PosAt>
__device__ __forceinline__ Threshold block_threshold(uint64_t M, uint32_t F, WordAt word_at, PosAt pos_at,
                                                     BlockSelLds &s) {
  const uint32_t tid = threadIdx.x;
  uint32_t prefix = 0, k = F;  // the k-th smallest (1-based) among the items whose decided high bits equal prefix's
  for (int shift = 24; shift >= 0; shift -= 8) {
    s.hist[tid] = 0;
    __syncthreads();
    for (uint64_t i = tid; i < M; i += kBlock) {
      const uint32_t w = word_at(i);
      if (shift == 24 || (w >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s.hist[(w >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t cnt = s.hist[tid];
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan<kWavesPerBlock>(cnt, s.scan, &tot);
    if (ex < k && k <= ex + cnt) {  // exactly one bin
      s.pick[0] = tid;
      s.pick[1] = k - ex;
    }
    __syncthreads();
    prefix |= s.pick[0] << shift;
    k = s.pick[1];
    __syncthreads();
  }
  // k of the items whose word equals prefix are kept, the first ones by position; usually there are exactly k
  const uint32_t equals = s.hist[prefix & 255u];
  __syncthreads();
  if (equals == k) return Threshold{prefix, 0xFFFFFFFFu};
  uint32_t seen = 0;
  for (uint64_t base = 0; base < M && seen < k; base += kBlock) {
    const uint64_t i = base + tid;
    const bool eq = i < M && word_at(i) == prefix;
    uint32_t tot;
    const uint32_t r = block_exclusive_rank<kWavesPerBlock>(eq, s.scan, &tot);
    if (eq && seen + r == k - 1) s.pick[0] = pos_at(i);
    seen += tot;
  }
  __syncthreads();
  const uint32_t j = s.pick[0];
  __syncthreads();
  return Threshold{prefix, j};
}

// emits the kept items in order: put(rank, i) for the rank-th kept item
template <typename WordAt, typename PosAt, typename Put>
__device__ __forceinline__ void block_emit(uint64_t M, Threshold th, WordAt word_at, PosAt pos_at, Put put,
                                           BlockSelLds &s) {
  uint32_t done = 0;
  for (uint64_t base = 0; base < M; base += kBlock) {
    const uint64_t i = base + threadIdx.x;
    bool take = false;
    if (i < M) {
      const uint32_t w = word_at(i);
      take = w < th.w || (w == th.w && pos_at(i) <= th.j);
    }
    uint32_t tot;
    const uint32_t r = block_exclusive_rank<kWavesPerBlock>(take, s.scan, &tot);
    if (take) put(done + r, i);
    done += tot;
  }
}

// ---- hub rows: list, then reduce every piece to its F smallest pairs ------------------------------------------------
__global__ void hub_reset_kernel(HubWs hub) {
  if (threadIdx.x == 0) {
    *hub.count = 0;
    *hub.end = 0;
    *hub.used = 0;
  }
}

__global__ __launch_bounds__(kBlock) void hub_scan_kernel(const uint32_t *__restrict__ indptr,
                                                          const uint32_t *__restrict__ input, size_t num_input,
                                                          const uint32_t *d_num_input, size_t cap, uint32_t F,
                                                          HubWs hub) {
  const size_t n = resolve_count(num_input, d_num_input, cap);
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cap) return;
  uint32_t h = FGNN_EMPTY_KEY;
  if (i < n) {
    const uint32_t rid = input[i];
    const uint32_t off = indptr[rid], len = indptr[rid + 1] - off;
    if (len > kBlockRow) {
      h = atomicAdd(hub.count, 1u);
      if (h < kMaxHubs) {
        const uint32_t pieces = (len - 1) / kBlockRow + 1;
        const unsigned long long need = (unsigned long long)pieces * F;
        const unsigned long long first = atomicAdd(hub.used, need);
        const bool room = first + need <= kHubPool;
        hub.list[4 * h] = off;
        hub.list[4 * h + 1] = len;
        hub.list[4 * h + 2] = room ? (uint32_t)first : 0u;
        hub.list[4 * h + 3] = room ? pieces : 0u;
        if (room) {  // claims are whole multiples of F pairs: piece q of this row is piece first / F + q of the pool
          atomicMax(hub.end, (uint32_t)(first + need));
          for (uint32_t q = 0; q < pieces; ++q) hub.piece_hub[(uint32_t)first / F + q] = h;
        } else {
          h = FGNN_EMPTY_KEY;
        }
      } else {
        h = FGNN_EMPTY_KEY;
      }
    }
  }
  hub.of_seed[i] = h;
}

__global__ __launch_bounds__(kBlock) void hub_piece_kernel(const uint32_t *__restrict__ indices, HubWs hub, uint32_t F,
                                                           uint64_t seed, uint64_t batch_key, uint32_t tag) {
  __shared__ uint32_t sh_w[kBlockRow];
  __shared__ BlockSelLds sel;
  const uint32_t tid = threadIdx.x;
  // the pieces of all listed rows form one flat index space: the pool's, in units of F pairs
  const uint32_t total = *hub.end / F;
  for (uint32_t p = blockIdx.x; p < total; p += gridDim.x) {
    const uint32_t a = hub.piece_hub[p];
    const uint32_t off = hub.list[4 * a], len = hub.list[4 * a + 1];
    const uint32_t q = p - hub.list[4 * a + 2] / F;
    const uint32_t lo = q * kBlockRow;
    const uint32_t m = len - lo < kBlockRow ? len - lo : kBlockRow;
    const size_t out = (size_t)hub.list[4 * a + 2] + (size_t)q * F;
    __syncthreads();  // the previous piece's words have been consumed
    for (uint32_t i = tid; i < m; i += kBlock) sh_w[i] = node_word(seed, batch_key, tag, indices[(size_t)off + lo + i]);
    __syncthreads();
    auto word_at = [&](uint64_t i) { return sh_w[i]; };
    auto pos_at = [&](uint64_t i) { return lo + (uint32_t)i; };
    if (m <= F) {  // a short last piece: all of it
      for (uint32_t i = tid; i < m; i += kBlock) {
        hub.cand_w[out + i] = sh_w[i];
        hub.cand_j[out + i] = lo + i;
      }
    } else {
      const Threshold th = block_threshold(m, F, word_at, pos_at, sel);
      block_emit(m, th, word_at, pos_at, [&](uint32_t r, uint64_t i) {
        hub.cand_w[out + r] = sh_w[i];
        hub.cand_j[out + r] = lo + (uint32_t)i;
      }, sel);
    }
  }
}

// ---- a wave-owned row: F < len <= kWaveRow ---------------------------------------------------------------------------
// t0: the row's first 64 entries (lane l: indices[off + l], loaded by the caller).  Writes F edges from position `o` on.
__device__ __forceinline__ void wave_row(const uint32_t *__restrict__ indices, uint32_t off, uint32_t len, uint32_t F,
                                         uint32_t t0, uint64_t seed, uint64_t batch_key, uint32_t tag, uint32_t src,
                                         uint32_t *__restrict__ out_src, uint32_t *__restrict__ out_dst, size_t o) {
  const uint32_t lane = (uint32_t)lane_id();
  uint32_t t[kRegs], w[kRegs];
  t[0] = t0;
#pragma unroll
  for (int i = 1; i < kRegs; ++i) {
    t[i] = 0;
    if ((uint32_t)i * kWave < len) {  // wave-uniform
      const uint32_t j = (uint32_t)i * kWave + lane;
      if (j < len) t[i] = indices[(size_t)off + j];
    }
  }
#pragma unroll
  for (int i = 0; i < kRegs; ++i) {
    w[i] = 0;
    if ((uint32_t)i * kWave < len) w[i] = node_word(seed, batch_key, tag, t[i]);
  }
  // the F-th smallest word, bit by bit: candidates agree with `prefix` above `bit`
  uint32_t prefix = 0, k = F;
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    uint32_t zeros = 0;
#pragma unroll
    for (int i = 0; i < kRegs; ++i) {
      if ((uint32_t)i * kWave < len) {
        const bool p = (uint32_t)i * kWave + lane < len && ((w[i] ^ prefix) >> bit) == 0u;
        zeros += (uint32_t)__popcll(__ballot(p));
      }
    }
    if (k > zeros) {
      k -= zeros;
      prefix |= 1u << bit;
    }
  }
  // k of the elements whose word equals prefix are kept, the first ones by position
  uint32_t tj = 0xFFFFFFFFu, seen = 0;
#pragma unroll
  for (int i = 0; i < kRegs; ++i) {
    if ((uint32_t)i * kWave < len) {
      unsigned long long m = __ballot((uint32_t)i * kWave + lane < len && w[i] == prefix);
      const uint32_t c = (uint32_t)__popcll(m);
      if (seen < k && seen + c >= k) {  // the k-th equal element is in this trip: its (k - seen)-th set bit
        for (uint32_t q = seen + 1; q < k; ++q) m &= m - 1;
        tj = (uint32_t)i * kWave + (uint32_t)__builtin_ctzll(m);
      }
      seen += c;
    }
  }
  uint32_t done = 0;
#pragma unroll
  for (int i = 0; i < kRegs; ++i) {
    if ((uint32_t)i * kWave < len) {
      const uint32_t j = (uint32_t)i * kWave + lane;
      const bool take = j < len && (w[i] < prefix || (w[i] == prefix && j <= tj));
      const unsigned long long m = __ballot(take);
      if (take) {
        const size_t at = o + done + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        out_dst[at] = t[i];
        out_src[at] = src;
      }
      done += (uint32_t)__popcll(m);
    }
  }
}

// ---- the sampler ---------------------------------------------------------------------------------------------------
// mode 0: single pass (offsets by the cross-workgroup prefix); 1: count only (block_sums[tile] = edges of the tile);
// 2: emit with the scanned block_sums as offsets
template <int S>
__global__ __launch_bounds__(kBlock) void khop_shared_kernel(const uint32_t *__restrict__ indptr,
                                                             const uint32_t *__restrict__ indices,
                                                             const uint32_t *__restrict__ input, size_t num_input,
                                                             const uint32_t *d_num_input, size_t cap, uint32_t F,
                                                             uint32_t *__restrict__ out_src,
                                                             uint32_t *__restrict__ out_dst, int src_mode,
                                                             uint64_t seed, uint64_t batch_key, uint32_t tag,
                                                             ScanWs scan, size_t *d_num_out, int mode,
                                                             uint32_t *__restrict__ block_sums, HubWs hub) {
  static_assert(S % kWavesPerBlock == 0 && S <= kBlock, "seeds per workgroup");
  __shared__ uint32_t sh_w[kBlockRow];
  __shared__ BlockSelLds sel;
  __shared__ uint32_t sh_off[S], sh_len[S], sh_rid[S], sh_lo[S], sh_hub[S];
  __shared__ uint32_t sh_big[S], sh_nbig;
  __shared__ uint32_t sh_tile[2];
  const uint32_t tid = threadIdx.x;
  const uint32_t tile = blockIdx.x;
  const size_t n = resolve_count(num_input, d_num_input, cap);
  const size_t first = (size_t)tile * S;
  const uint32_t last_tile = n ? (uint32_t)((n - 1) / S) : 0u;
  if (tile > last_tile) {  // no seeds here and nobody waits for this tile
    if (mode == 1 && tid == 0) block_sums[tile] = 0;
    return;
  }
  if (tid == 0) sh_nbig = 0;
  __syncthreads();
  uint32_t c = 0;
  if (tid < S) {
    uint32_t rid = 0, off = 0, len = 0, h = FGNN_EMPTY_KEY;
    if (first + tid < n) {
      rid = input[first + tid];
      off = indptr[rid];
      len = indptr[rid + 1] - off;
      if (mode != 1 && len > kBlockRow) h = hub.of_seed[first + tid];
      if (mode != 1 && len > kWaveRow) sh_big[atomicAdd(&sh_nbig, 1u)] = tid;
    }
    c = len < F ? len : F;
    sh_off[tid] = off;
    sh_len[tid] = len;
    sh_rid[tid] = rid;
    sh_hub[tid] = h;
  }
  uint32_t total;
  const uint32_t lo = block_exclusive_scan<kWavesPerBlock>(c, sel.scan, &total);
  if (tid < S) sh_lo[tid] = lo;
  if (mode == 1) {
    if (tid == 0) block_sums[tile] = total;
    return;
  }
  size_t base;
  if (mode == 0) {
    // every tile publishes before it touches a row, so the wait is short; a waiter that outlasts the poll budget
    // recomputes a missing tile's edge count itself: min(len, F) over the tile's seeds, from immutable inputs
    scan_publish_aggregate(scan, tile, total);
    base = scan_prefix_help(scan, tile, sh_tile, [&](uint32_t m) -> uint32_t {
      uint32_t cm = 0;
      const size_t im = (size_t)m * S + tid;
      if (tid < S && im < n) {
        const uint32_t r = input[im];
        const uint32_t l = indptr[r + 1] - indptr[r];
        cm = l < F ? l : F;
      }
      uint32_t tot_m;
      (void)block_exclusive_scan<kWavesPerBlock>(cm, sel.scan, &tot_m);
      return tot_m;
    });
    if (tile == last_tile && tid == 0 && d_num_out) *d_num_out = base + total;
  } else {
    base = block_sums[tile];
  }
  __syncthreads();  // sh_lo, sh_big

  // ---- rows of up to kWaveRow entries: wave v takes seeds v, v + 4, ... ---------------------------------------------
  const uint32_t lane = (uint32_t)lane_id();
  uint32_t k = (uint32_t)wave_id();
  uint32_t t_next = 0;
  if (k < S && lane < sh_len[k] && sh_len[k] <= kWaveRow) t_next = indices[(size_t)sh_off[k] + lane];
  for (; k < S; k += kWavesPerBlock) {
    const uint32_t off = sh_off[k], len = sh_len[k];
    const uint32_t t0 = t_next;
    const uint32_t kn = k + kWavesPerBlock;
    t_next = 0;
    if (kn < S && lane < sh_len[kn] && sh_len[kn] <= kWaveRow) t_next = indices[(size_t)sh_off[kn] + lane];
    if (len == 0 || len > kWaveRow) continue;  // wave-uniform
    const uint32_t src = src_mode == FGNN_SRC_LOCAL ? (uint32_t)(first + k) : sh_rid[k];
    const size_t o = base + sh_lo[k];
    if (len <= F) {
      if (lane < len) {  // F <= 64: one trip
        out_dst[o + lane] = t0;
        out_src[o + lane] = src;
      }
    } else {
      wave_row(indices, off, len, F, t0, seed, batch_key, tag, src, out_src, out_dst, o);
    }
  }

  // ---- longer rows: the workgroup, one row after the other ----------------------------------------------------------
  const uint32_t nbig = sh_nbig;
  for (uint32_t b = 0; b < nbig; ++b) {
    const uint32_t kb = sh_big[b];
    const uint32_t off = sh_off[kb], len = sh_len[kb], h = sh_hub[kb];
    const uint32_t src = src_mode == FGNN_SRC_LOCAL ? (uint32_t)(first + kb) : sh_rid[kb];
    const size_t o = base + sh_lo[kb];
    const uint32_t *row = indices + off;
    auto put = [&](uint32_t r, uint32_t j) {
      out_dst[o + r] = row[j];
      out_src[o + r] = src;
    };
    __syncthreads();  // sh_w of the previous row has been consumed
    if (len <= kBlockRow) {
      for (uint32_t i = tid; i < len; i += kBlock) sh_w[i] = node_word(seed, batch_key, tag, row[i]);
      __syncthreads();
      auto word_at = [&](uint64_t i) { return sh_w[i]; };
      auto pos_at = [&](uint64_t i) { return (uint32_t)i; };
      const Threshold th = block_threshold(len, F, word_at, pos_at, sel);
      block_emit(len, th, word_at, pos_at, [&](uint32_t r, uint64_t i) { put(r, (uint32_t)i); }, sel);
    } else if (h != FGNN_EMPTY_KEY) {  // the whole chip left the candidates of this row's pieces in the pool
      const uint32_t at = hub.list[4 * h + 2], pieces = hub.list[4 * h + 3];
      const uint32_t last = len - (pieces - 1) * kBlockRow;
      const uint64_t M = (uint64_t)(pieces - 1) * F + (last < F ? last : F);
      const uint32_t *cw = hub.cand_w + at, *cj = hub.cand_j + at;
      auto word_at = [&](uint64_t i) { return cw[i]; };
      auto pos_at = [&](uint64_t i) { return cj[i]; };
      const Threshold th = block_threshold(M, F, word_at, pos_at, sel);
      block_emit(M, th, word_at, pos_at, [&](uint32_t r, uint64_t i) { put(r, cj[i]); }, sel);
    } else {  // a hub without room in the pool: stream the row, the words recomputed in every pass
      auto word_at = [&](uint64_t i) { return node_word(seed, batch_key, tag, row[i]); };
      auto pos_at = [&](uint64_t i) { return (uint32_t)i; };
      const Threshold th = block_threshold(len, F, word_at, pos_at, sel);
      block_emit(len, th, word_at, pos_at, [&](uint32_t r, uint64_t i) { put(r, (uint32_t)i); }, sel);
    }
  }
}

// scratch, in 4-byte words: block sums | hub index per seed | hub header (8) | hub list | candidate pool (two arrays) |
// piece map
struct WsLayout { size_t sums, of_seed, header, list, cand_w, cand_j, piece_hub, words; };
inline WsLayout ws_layout(size_t cap) {
  WsLayout l;
  l.sums = 0;
  l.of_seed = (div_up(cap, (size_t)64) + 8 + 1) & ~(size_t)1;
  l.header = (l.of_seed + cap + 1) & ~(size_t)1;  // holds a 64-bit counter
  l.list = l.header + 8;
  l.cand_w = l.list + 4 * (size_t)kMaxHubs;
  l.cand_j = l.cand_w + kHubPool;
  l.piece_hub = l.cand_j + kHubPool;
  l.words = l.piece_hub + kHubPool;
  return l;
}

}  // namespace

int sample_khop_shared(const LayerCall &c, ScanWsHost *scan_host) {
  if (c.fanout == 0 || c.fanout > kMaxFanout) return FGNN_EINVAL;
  const LayerPrologue pro = layer_prologue(c, FGNN_KHOP_SHARED);
  if (pro.empty) return pro.rc;
  const size_t cap = pro.cap;
  if (!c.indptr || !c.indices || !c.input || !c.out_src || !c.out_dst || cap * c.fanout >= 0x7fffffffull)
    return FGNN_EINVAL;
  const WsLayout lay = ws_layout(cap);
  if (!c.ws || c.ws_bytes < lay.words * sizeof(uint32_t)) return FGNN_ENOSPC;
  if (reinterpret_cast<uintptr_t>(c.ws) & 7u) return FGNN_EINVAL;
  const uint32_t F = (uint32_t)c.fanout;
  const hipStream_t st = c.stream;
  uint32_t *const ws = static_cast<uint32_t *>(c.ws);
  uint32_t *const sums = ws + lay.sums;
  const HubWs hub{ws + lay.of_seed, ws + lay.header, ws + lay.header + 1,
                  reinterpret_cast<unsigned long long *>(ws + lay.header + 2), ws + lay.list, ws + lay.cand_w,
                  ws + lay.cand_j, ws + lay.piece_hub};
  // small frontiers: small tiles, more workgroups to hide the row loads behind
  const int S = div_up(cap, (size_t)64) <= kSinglePassMaxTiles ? 64 : 256;
  const size_t nb = div_up(cap, (size_t)S);
  hipLaunchKernelGGL(hub_reset_kernel, dim3(1), dim3(kWave), 0, st, hub);
  hipLaunchKernelGGL(hub_scan_kernel, dim3(div_up(cap, (size_t)kBlock)), dim3(kBlock), 0, st, c.indptr, c.input,
                     c.num_input, c.d_num_input, cap, F, hub);
  hipLaunchKernelGGL(hub_piece_kernel, dim3((unsigned)device_cu_count() * 4), dim3(kBlock), 0, st, c.indices, hub, F,
                     c.seed, c.batch_key, pro.tag);
  ScanWs scan{nullptr, nullptr, 0, 0, nullptr, nullptr, 0, kScanHelpAfterPolls, nullptr};
  const bool single = scan_host && nb <= kSinglePassMaxTiles && nb <= scan_host->ws.max_tiles;
  if (single) scan = scan_host->next(0, nb);
#define FGNN_KS(SS, MODE)                                                                                          \
  hipLaunchKernelGGL((khop_shared_kernel<SS>), dim3(nb), dim3(kBlock), 0, st, c.indptr, c.indices, c.input,        \
                     c.num_input, c.d_num_input, cap, F, c.out_src, c.out_dst, c.src_mode, c.seed, c.batch_key,    \
                     pro.tag, scan, c.d_num_out, MODE, sums, hub)
#define FGNN_KS_MODE(MODE)      \
  do {                          \
    if (S == 64) FGNN_KS(64, MODE); \
    else FGNN_KS(256, MODE);    \
  } while (0)
  if (single) {
    FGNN_KS_MODE(0);
  } else {
    FGNN_KS_MODE(1);
    if (launch_scan_block_sums(sums, nb, c.d_num_out, nullptr, nullptr, nullptr, st) != FGNN_OK) return FGNN_EHIP;
    FGNN_KS_MODE(2);
  }
#undef FGNN_KS_MODE
#undef FGNN_KS
  return launch_status(__func__);
}

}  // namespace fgnn

extern "C" size_t fgnn_khop_shared_scratch_bytes(size_t num_input_cap, size_t fanout) {
  (void)fanout;  // the candidate pool is sized for the largest fanout
  return fgnn::ws_layout(num_input_cap).words * sizeof(uint32_t);
}

extern "C" void fgnn_khop_shared_params(uint32_t out[3]) {
  out[0] = fgnn::kMaxFanout;
  out[1] = fgnn::kWaveRow;
  out[2] = fgnn::kBlockRow;
}

extern "C" void fgnn_khop_shared_pool_params(uint32_t out[2]) {
  out[0] = fgnn::kMaxHubs;
  out[1] = fgnn::kHubPool;
}

extern "C" int fgnn_debug_khop_shared_hub_state(const void *ws, size_t num_input_cap, unsigned long long out[3]) {
  if (!ws || !num_input_cap || !out || (reinterpret_cast<uintptr_t>(ws) & 7u)) return FGNN_EINVAL;
  FGNN_HIP_CHECK(hipDeviceSynchronize());
  uint32_t header[4];  // count, end, used (64 bits)
  FGNN_HIP_CHECK(hipMemcpy(header, static_cast<const uint32_t *>(ws) + fgnn::ws_layout(num_input_cap).header,
                           sizeof(header), hipMemcpyDeviceToHost));
  out[0] = header[0];
  out[1] = header[1];
  out[2] = (unsigned long long)header[3] << 32 | header[2];
  return FGNN_OK;
}

extern "C" int fgnn_sample_khop_shared(const uint32_t *indptr, const uint32_t *indices, const uint32_t *input,
                                       size_t num_input, const uint32_t *d_num_input, size_t num_input_cap,
                                       size_t fanout, uint32_t *out_src, uint32_t *out_dst, size_t *d_num_out,
                                       int src_mode, uint64_t seed, uint64_t batch_key, uint32_t layer, void *ws,
                                       size_t ws_bytes, void *stream) {
  return fgnn::sample_khop_shared(
      fgnn::LayerCall{indptr, const_cast<uint32_t *>(indices), input, num_input, d_num_input, num_input_cap, fanout,
                      out_src, out_dst, d_num_out, src_mode, seed, batch_key, layer, ws, ws_bytes,
                      static_cast<hipStream_t>(stream)},
      nullptr);
}
