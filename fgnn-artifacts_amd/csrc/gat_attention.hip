// gat_attention.hip -- the attention aggregation of a GAT layer over a sampled block (examples/models.py: FusedGATConv;
// reference: dgl.nn.GATConv as example/samgraph/train_gat.py uses it).  H heads of F features, D = H F:
//     s[e,h] = leaky_relu(el[row[e],h] + er[col[e],h])          a[e,h] = softmax of s over the edges of col[e]
//     out[col[e],h,:] += a~[e,h] feat[row[e],h,:]                a~ = a * keep / (1 - q)   (attention dropout)
// Op by op this materialises feat[row] (E x H x F) twice per layer and direction; here nothing wider than E x H is ever
// written.  Every pass is independent of the order of the edges (a destination's edges need not be contiguous):
//   forward    zero m, z | scores + segment max | exp + segment sum | normalise (+ dropout mask) | aggregation
//   backward   zero t | edge dot products ga = <g[col], feat[row]> | mask, t = sum a ga | gs, gel, ger | aggregation of
//              g[col] into gfeat[row] (the forward's kernel with the index arrays swapped)
// The per-(destination, head) max and sums are atomics on E x H values collapsed per wave: one lane per edge, a ballot
// of the run heads, a segmented wave scan, one atomic per (wave, run of equal destinations, head) -- seed-major blocks
// have a few runs per wave, an unsorted block only has short runs.  The float max is an unsigned integer max over a
// monotone encoding of the float whose zero lies below every float, so one zero fill initialises max and sum alike.
// The aggregation is block_aggregate_kernel's shape (a wave owns 32 edges and broadcasts their indices by shuffle, lane
// l owns columns l + 64 q, sums stay in registers while the destination does not change); the weight of column c is
// a~[e, c / F], the lane's heads are computed once per trip.  fp32; the order of the additions is not fixed.
#include "fgnn_device.h"

namespace fgnn {
namespace {

// monotone float -> uint32 (a < b  <=>  key(a) < key(b) for non-NaN floats); key 0 decodes to a NaN below everything
__device__ __forceinline__ uint32_t float_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// One edge per lane: the runs of equal destinations over a wave's live lanes (the first `cnt`).  `first` = the lane
// that starts this lane's run, `tail` = this lane ends its run (it issues the run's atomic).
struct Runs {
  uint32_t first;
  bool tail;
};

__device__ __forceinline__ Runs wave_runs(uint32_t key, bool live, uint32_t lane) {
  const uint32_t prev = __shfl_up(key, 1, kWave);
  const bool head = live && (lane == 0 || prev != key);
  const unsigned long long heads = __ballot(head);
  const uint32_t cnt = (uint32_t)__popcll(__ballot(live));
  const unsigned long long below = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
  Runs r;
  r.first = below ? 63u - (uint32_t)__builtin_clzll(below) : 0u;
  r.tail = live && (lane + 1 == cnt || ((heads >> (lane + 1)) & 1ull));
  return r;
}

// inclusive scans inside a run (dead lanes sit above the live ones and are never read by them)
__device__ __forceinline__ float run_sum(float s, uint32_t first, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const float t = __shfl_up(s, d, kWave);
    if (lane >= first + (uint32_t)d) s += t;
  }
  return s;
}
__device__ __forceinline__ float run_max(float s, uint32_t first, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const float t = __shfl_up(s, d, kWave);
    if (lane >= first + (uint32_t)d) s = fmaxf(s, t);
  }
  return s;
}

// keep iff the element's Philox word >= p 2^32: the keying and the rule of relu_dropout_kernel, element = e H + h
__device__ __forceinline__ uint32_t drop_threshold(float p) {
  return p <= 0.f ? 0u : (uint32_t)((double)p * 4294967296.0);
}
__device__ __forceinline__ bool keep_element(size_t idx, uint32_t thr, uint64_t seed, unsigned long long step,
                                             uint32_t tag) {
  const size_t t = idx >> 2;
  return pick_word(philox_block(seed, step, tag, (uint32_t)t, (uint32_t)(t >> 32)), (uint32_t)(idx & 3u)) >= thr;
}

__global__ __launch_bounds__(kBlock) void gat_zero_kernel(float *p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) p[i] = 0.0f;
}

// pass 1: sc[e,h] = leaky_relu(el[row] + er[col]); mkey[col,h] = max (encoded)
__global__ __launch_bounds__(kBlock) void gat_score_max_kernel(const uint32_t *__restrict__ src_idx,
                                                               const uint32_t *__restrict__ dst_idx,
                                                               const float *__restrict__ el,
                                                               const float *__restrict__ er, size_t num_edge,
                                                               uint32_t H, float slope, float *__restrict__ sc,
                                                               uint32_t *mkey) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = (uint32_t)lane_id();
  const bool live = e < num_edge;
  if (__ballot(live) == 0ull) return;  // wave-uniform
  uint32_t row = 0, col = 0;
  if (live) {
    row = src_idx[e];
    col = dst_idx[e];
  }
  const Runs r = wave_runs(col, live, lane);
  for (uint32_t h = 0; h < H; ++h) {
    float s = -__builtin_inff();
    if (live) {
      const float x = el[(size_t)row * H + h] + er[(size_t)col * H + h];
      s = x > 0.0f ? x : slope * x;
      sc[e * H + h] = s;
    }
    const float m = run_max(s, r.first, lane);
    if (r.tail) atomicMax(&mkey[(size_t)col * H + h], float_key(m));
  }
}

// pass 2: sc[e,h] = exp(sc[e,h] - m[col,h]); z[col,h] += it
__global__ __launch_bounds__(kBlock) void gat_exp_sum_kernel(const uint32_t *__restrict__ dst_idx, size_t num_edge,
                                                             uint32_t H, float *__restrict__ sc,
                                                             const uint32_t *__restrict__ mkey, float *z) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = (uint32_t)lane_id();
  const bool live = e < num_edge;
  if (__ballot(live) == 0ull) return;
  const uint32_t col = live ? dst_idx[e] : 0u;
  const Runs r = wave_runs(col, live, lane);
  for (uint32_t h = 0; h < H; ++h) {
    float p = 0.0f;
    if (live) {
      p = expf(sc[e * H + h] - key_float(mkey[(size_t)col * H + h]));
      sc[e * H + h] = p;
    }
    const float s = run_sum(p, r.first, lane);
    if (r.tail) unsafeAtomicAdd(&z[(size_t)col * H + h], s);
  }
}

// pass 3: alpha = p / z[col]; aw = alpha * keep / (1 - q) when a mask is drawn (aw == null: none).  A thread takes
// the four elements of one Philox block; E H need not be a multiple of 4.
__global__ __launch_bounds__(kBlock) void gat_normalise_kernel(const uint32_t *__restrict__ dst_idx, size_t total,
                                                               uint32_t H, const float *__restrict__ sc,
                                                               const float *__restrict__ z, float *__restrict__ alpha,
                                                               float *__restrict__ aw, float p, float scale,
                                                               uint64_t seed,
                                                               const unsigned long long *__restrict__ d_step,
                                                               uint32_t tag) {
  const unsigned long long step = d_step ? *d_step : 0ull;
  const uint32_t thr = drop_threshold(p);
  const size_t n4 = (total + 3) / 4;
  for (size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x; t < n4; t += (size_t)gridDim.x * kBlock) {
    u32x4 r = {0u, 0u, 0u, 0u};
    if (aw) r = philox_block(seed, step, tag, (uint32_t)t, (uint32_t)(t >> 32));
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const size_t idx = 4 * t + j;
      if (idx >= total) break;
      const size_t e = idx / H;
      const uint32_t h = (uint32_t)(idx - e * H);
      const float a = sc[idx] / z[(size_t)dst_idx[e] * H + h];
      alpha[idx] = a;
      if (aw) aw[idx] = pick_word(r, j) >= thr ? a * scale : 0.0f;
    }
  }
}

// out[dst[e], c] += wgt[e, c / F] * h[src[e], c]: block_aggregate_kernel with a weight per (edge, head).  Lane l owns
// columns l + 64 q of a trip; its heads are fixed for the trip, the weights of an edge are loaded beside its row.
template <int P>
__global__ __launch_bounds__(kBlock) void gat_aggregate_kernel(const uint32_t *__restrict__ src_idx,
                                                               const uint32_t *__restrict__ dst_idx,
                                                               const float *__restrict__ wgt,
                                                               const float *__restrict__ h, float *out, size_t num_edge,
                                                               uint32_t H, uint32_t F, uint32_t dim, uint32_t h_ld,
                                                               uint32_t out_ld) {
  const size_t wave = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  const size_t e0 = wave * kEdgesPerWave;
  if (e0 >= num_edge) return;  // wave-uniform
  const size_t e1 = e0 + kEdgesPerWave < num_edge ? e0 + kEdgesPerWave : num_edge;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t cnt = (uint32_t)(e1 - e0);
  uint32_t my_src = 0, my_dst = 0;
  if (lane < cnt) {
    my_src = src_idx[e0 + lane];
    my_dst = dst_idx[e0 + lane];
  }
  const float *wchunk = wgt + e0 * H;
  for (uint32_t dbase = 0; dbase < dim; dbase += kWave * P) {  // one trip for dim <= 64 P
    bool act[P];
    float acc[P];
    uint32_t head[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const uint32_t c = dbase + lane + kWave * q;
      act[q] = c < dim;
      head[q] = act[q] ? c / F : 0u;
      acc[q] = 0.0f;
    }
    uint32_t cur = __shfl(my_dst, 0, kWave);
    constexpr uint32_t UN = 4;  // edges whose row loads are in flight together
    for (uint32_t i0 = 0; i0 < cnt; i0 += UN) {
      float v[UN][P], we[UN][P];
      uint32_t c[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t i = i0 + u < cnt ? i0 + u : cnt - 1;  // clamp: the extra loads are discarded below
        const uint32_t sidx = __shfl(my_src, (int)i, kWave);
        c[u] = __shfl(my_dst, (int)i, kWave);
        const float *hp = h + (size_t)sidx * h_ld + dbase + lane;
        const float *wp = wchunk + (size_t)i * H;
#pragma unroll
        for (int q = 0; q < P; ++q) {
          v[u][q] = act[q] ? hp[kWave * q] : 0.0f;
          we[u][q] = act[q] ? wp[head[q]] : 0.0f;
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (i0 + u >= cnt) break;  // wave-uniform
        if (c[u] != cur) {         // wave-uniform: segment boundary, flush
          float *op = out + (size_t)cur * out_ld + dbase + lane;
#pragma unroll
          for (int q = 0; q < P; ++q) {
            if (act[q]) unsafeAtomicAdd(op + kWave * q, acc[q]);
            acc[q] = 0.0f;
          }
          cur = c[u];
        }
#pragma unroll
        for (int q = 0; q < P; ++q) acc[q] += we[u][q] * v[u][q];
      }
    }
    float *op = out + (size_t)cur * out_ld + dbase + lane;
#pragma unroll
    for (int q = 0; q < P; ++q)
      if (act[q]) unsafeAtomicAdd(op + kWave * q, acc[q]);
  }
}

// ga[e,h] = <g[col[e],h,:], feat[row[e],h,:]> for F a power of two <= 64: the aggregation's shape (a wave owns 32
// edges, lane l owns columns l + 64 q), every row is read once with full-width loads, and the F lanes of a head -- an
// aligned group, since F divides 64 and every trip starts at a multiple of 64 -- reduce their products by xor shuffles.
template <int P>
__global__ __launch_bounds__(kBlock) void gat_edge_dot_pow2_kernel(const uint32_t *__restrict__ src_idx,
                                                                   const uint32_t *__restrict__ dst_idx,
                                                                   const float *__restrict__ feat,
                                                                   const float *__restrict__ g,
                                                                   float *__restrict__ ga, size_t num_edge, uint32_t H,
                                                                   uint32_t F, uint32_t dim, uint32_t feat_ld,
                                                                   uint32_t g_ld) {
  const size_t wave = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  const size_t e0 = wave * kEdgesPerWave;
  if (e0 >= num_edge) return;  // wave-uniform
  const size_t e1 = e0 + kEdgesPerWave < num_edge ? e0 + kEdgesPerWave : num_edge;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t cnt = (uint32_t)(e1 - e0);
  uint32_t my_src = 0, my_dst = 0;
  if (lane < cnt) {
    my_src = src_idx[e0 + lane];
    my_dst = dst_idx[e0 + lane];
  }
  const bool writer = (lane & (F - 1u)) == 0u;
  for (uint32_t dbase = 0; dbase < dim; dbase += kWave * P) {
    bool act[P];
    uint32_t head[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const uint32_t c = dbase + lane + kWave * q;
      act[q] = c < dim;
      head[q] = act[q] ? c / F : 0u;
    }
    constexpr uint32_t UN = 2;  // edges in flight: two rows each
    for (uint32_t i0 = 0; i0 < cnt; i0 += UN) {
      float prod[UN][P];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t i = i0 + u < cnt ? i0 + u : cnt - 1;
        const uint32_t sidx = __shfl(my_src, (int)i, kWave);
        const uint32_t didx = __shfl(my_dst, (int)i, kWave);
        const float *fp = feat + (size_t)sidx * feat_ld + dbase + lane;
        const float *gp = g + (size_t)didx * g_ld + dbase + lane;
#pragma unroll
        for (int q = 0; q < P; ++q) prod[u][q] = act[q] ? gp[kWave * q] * fp[kWave * q] : 0.0f;
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (i0 + u >= cnt) break;  // wave-uniform
#pragma unroll
        for (int q = 0; q < P; ++q) {
          float s = prod[u][q];
          for (uint32_t d = F >> 1; d > 0; d >>= 1) s += __shfl_xor(s, (int)d, kWave);  // wave-uniform trip count
          if (writer && act[q]) ga[(e0 + i0 + u) * H + head[q]] = s;
        }
      }
    }
  }
}

// the same for every other F: one thread per (edge, head) walks the head's F columns of both rows
__global__ __launch_bounds__(kBlock) void gat_edge_dot_kernel(const uint32_t *__restrict__ src_idx,
                                                              const uint32_t *__restrict__ dst_idx,
                                                              const float *__restrict__ feat,
                                                              const float *__restrict__ g, float *__restrict__ ga,
                                                              size_t total, uint32_t H, uint32_t F, uint32_t feat_ld,
                                                              uint32_t g_ld) {
  for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kBlock) {
    const size_t e = idx / H;
    const uint32_t h = (uint32_t)(idx - e * H);
    const float *fp = feat + (size_t)src_idx[e] * feat_ld + (size_t)h * F;
    const float *gp = g + (size_t)dst_idx[e] * g_ld + (size_t)h * F;
    float s = 0.0f;
    for (uint32_t f = 0; f < F; ++f) s += gp[f] * fp[f];
    ga[idx] = s;
  }
}

// backward, per (edge, head): the mask of the forward pass again (same key), aw = alpha keep / (1 - q) for the
// feature gradient's aggregation, and -- when el / er gradients are wanted (ga != null) -- ga *= keep / (1 - q) and
// t[col,h] += alpha ga
__global__ __launch_bounds__(kBlock) void gat_mask_t_kernel(const uint32_t *__restrict__ dst_idx, size_t num_edge,
                                                            uint32_t H, const float *__restrict__ alpha, float *ga,
                                                            float *__restrict__ aw, float *t, float p, float scale,
                                                            uint64_t seed,
                                                            const unsigned long long *__restrict__ d_step,
                                                            uint32_t tag) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = (uint32_t)lane_id();
  const bool live = e < num_edge;
  if (__ballot(live) == 0ull) return;
  const unsigned long long step = d_step ? *d_step : 0ull;
  const uint32_t thr = drop_threshold(p);
  const uint32_t col = live ? dst_idx[e] : 0u;
  const Runs r = wave_runs(col, live, lane);
  for (uint32_t h = 0; h < H; ++h) {
    float v = 0.0f;
    if (live) {
      const size_t idx = e * H + h;
      const float a = alpha[idx];
      float ks = 1.0f;
      if (aw) {
        ks = keep_element(idx, thr, seed, step, tag) ? scale : 0.0f;
        aw[idx] = a * ks;
      }
      if (ga) {
        const float gah = ga[idx] * ks;
        ga[idx] = gah;
        v = a * gah;
      }
    }
    if (ga) {  // kernel-uniform
      const float s = run_sum(v, r.first, lane);
      if (r.tail) unsafeAtomicAdd(&t[(size_t)col * H + h], s);
    }
  }
}

// gs = alpha (ga - t[col]); gpre = gs * (1 or slope by the sign of el + er); gel[row] += gpre, ger[col] += gpre
__global__ __launch_bounds__(kBlock) void gat_score_grad_kernel(const uint32_t *__restrict__ src_idx,
                                                                const uint32_t *__restrict__ dst_idx,
                                                                const float *__restrict__ el,
                                                                const float *__restrict__ er, size_t num_edge,
                                                                uint32_t H, float slope,
                                                                const float *__restrict__ alpha,
                                                                const float *__restrict__ ga,
                                                                const float *__restrict__ t, float *gel, float *ger) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = (uint32_t)lane_id();
  const bool live = e < num_edge;
  if (__ballot(live) == 0ull) return;
  uint32_t row = 0, col = 0;
  if (live) {
    row = src_idx[e];
    col = dst_idx[e];
  }
  const Runs r = wave_runs(col, live, lane);
  for (uint32_t h = 0; h < H; ++h) {
    float gpre = 0.0f;
    if (live) {
      const size_t idx = e * H + h;
      const float gs = alpha[idx] * (ga[idx] - t[(size_t)col * H + h]);
      const float x = el[(size_t)row * H + h] + er[(size_t)col * H + h];
      gpre = x > 0.0f ? gs : slope * gs;
      if (gel) unsafeAtomicAdd(&gel[(size_t)row * H + h], gpre);
    }
    if (ger) {  // kernel-uniform
      const float s = run_sum(gpre, r.first, lane);
      if (r.tail) unsafeAtomicAdd(&ger[(size_t)col * H + h], s);
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------

// workspace, in floats: m (encoded max) | z | t, num_dst H each; per-edge scores / dot products | dropped-out weights,
// num_edge H each
struct GatWs {
  uint32_t *mkey;
  float *z, *t, *sc, *aw;
};

inline size_t gat_ws_floats(size_t num_edge, size_t num_dst, size_t num_head) {
  return 3 * num_dst * num_head + 2 * num_edge * num_head;
}

inline GatWs gat_ws(void *ws, size_t num_edge, size_t num_dst, size_t num_head) {
  float *p = static_cast<float *>(ws);
  const size_t nd = num_dst * num_head, ne = num_edge * num_head;
  return GatWs{reinterpret_cast<uint32_t *>(p), p + nd, p + 2 * nd, p + 3 * nd, p + 3 * nd + ne};
}

inline unsigned capped_grid(size_t items) {
  const size_t want = div_up(items, (size_t)kBlock), cap = (size_t)device_cu_count() * 16;
  return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

// what both entry points refuse before any launch; the grids of the per-edge kernels on the way
bool gat_args_ok(const uint32_t *src_index, const uint32_t *dst_index, size_t num_edge, const float *el,
                 const float *er, const float *feat, size_t feat_ld, size_t num_dst, size_t num_head, size_t num_feat,
                 float attn_p, const void *ws, size_t ws_bytes) {
  if (!src_index || !dst_index || !el || !er || !feat || !ws || num_head == 0 || num_feat == 0) return false;
  if (!fits_u32(num_head) || !fits_u32(num_feat) || !fits_u32(num_head * num_feat) || !fits_u32(num_dst) ||
      feat_ld < num_head * num_feat || !fits_u32(feat_ld) || !(attn_p >= 0.f && attn_p < 1.f))
    return false;
  if (!float_aligned(src_index) || !float_aligned(dst_index) || !float_aligned(el) || !float_aligned(er) ||
      !float_aligned(feat) || !float_aligned(ws))
    return false;
  if (ws_bytes < fgnn_gat_workspace_bytes(num_edge, num_dst, num_head)) return false;
  return div_up(num_edge, (size_t)kEdgesPerWave * kWavesPerBlock) <= 0x7fffffffull;
}

void launch_gat_aggregate(const uint32_t *src_index, const uint32_t *dst_index, const float *wgt, const float *h,
                          size_t h_ld, float *out, size_t out_ld, size_t num_edge, size_t H, size_t F, hipStream_t st) {
  const size_t dim = H * F;
  const size_t blocks = div_up(div_up(num_edge, (size_t)kEdgesPerWave), (size_t)kWavesPerBlock);
  using Kernel = decltype(&gat_aggregate_kernel<1>);
  static constexpr Kernel kernels[3] = {gat_aggregate_kernel<1>, gat_aggregate_kernel<2>, gat_aggregate_kernel<4>};
  hipLaunchKernelGGL(kernels[dim <= 64 ? 0 : (dim <= 128 ? 1 : 2)], dim3(blocks), dim3(kBlock), 0, st, src_index,
                     dst_index, wgt, h, out, num_edge, (uint32_t)H, (uint32_t)F, (uint32_t)dim, (uint32_t)h_ld,
                     (uint32_t)out_ld);
}

}  // namespace
}  // namespace fgnn

extern "C" size_t fgnn_gat_workspace_bytes(size_t num_edge, size_t num_dst, size_t num_head) {
  return fgnn::gat_ws_floats(num_edge, num_dst, num_head) * sizeof(float);
}

extern "C" int fgnn_gat_forward(const uint32_t *src_index, const uint32_t *dst_index, size_t num_edge, const float *el,
                                const float *er, const float *feat, size_t feat_ld, size_t num_dst, size_t num_head,
                                size_t num_feat, float negative_slope, float attn_p, uint64_t seed,
                                const unsigned long long *d_step, uint32_t tag, float *alpha, float *out, size_t out_ld,
                                void *ws, size_t ws_bytes, void *stream) {
  using namespace fgnn;
  if (num_edge == 0) return FGNN_OK;
  if (!gat_args_ok(src_index, dst_index, num_edge, el, er, feat, feat_ld, num_dst, num_head, num_feat, attn_p, ws,
                   ws_bytes))
    return FGNN_EINVAL;
  if (!alpha || !out || out_ld < num_head * num_feat || !fits_u32(out_ld) || !float_aligned(alpha) ||
      !float_aligned(out) || !float_aligned(d_step))
    return FGNN_EINVAL;
  auto st = static_cast<hipStream_t>(stream);
  const GatWs w = gat_ws(ws, num_edge, num_dst, num_head);
  const uint32_t H = (uint32_t)num_head;
  const size_t total = num_edge * num_head;
  const unsigned edge_blocks = (unsigned)div_up(num_edge, (size_t)kBlock);
  const bool drop = attn_p > 0.f;
  hipLaunchKernelGGL(gat_zero_kernel, dim3(capped_grid(2 * num_dst * num_head)), dim3(kBlock), 0, st,
                     reinterpret_cast<float *>(w.mkey), 2 * num_dst * num_head);  // m and z
  hipLaunchKernelGGL(gat_score_max_kernel, dim3(edge_blocks), dim3(kBlock), 0, st, src_index, dst_index, el, er,
                     num_edge, H, negative_slope, w.sc, w.mkey);
  hipLaunchKernelGGL(gat_exp_sum_kernel, dim3(edge_blocks), dim3(kBlock), 0, st, dst_index, num_edge, H, w.sc, w.mkey,
                     w.z);
  hipLaunchKernelGGL(gat_normalise_kernel, dim3(capped_grid(div_up(total, (size_t)4))), dim3(kBlock), 0, st, dst_index,
                     total, H, w.sc, w.z, alpha, drop ? w.aw : nullptr, attn_p, 1.0f / (1.0f - attn_p), seed, d_step,
                     tag);
  launch_gat_aggregate(src_index, dst_index, drop ? w.aw : alpha, feat, feat_ld, out, out_ld, num_edge, num_head,
                       num_feat, st);
  return launch_status(__func__);
}

extern "C" int fgnn_gat_backward(const uint32_t *src_index, const uint32_t *dst_index, size_t num_edge, const float *el,
                                 const float *er, const float *feat, size_t feat_ld, const float *alpha,
                                 const float *gout, size_t gout_ld, size_t num_dst, size_t num_head, size_t num_feat,
                                 float negative_slope, float attn_p, uint64_t seed, const unsigned long long *d_step,
                                 uint32_t tag, float *gfeat, size_t gfeat_ld, float *gel, float *ger, void *ws,
                                 size_t ws_bytes, void *stream) {
  using namespace fgnn;
  if (num_edge == 0) return FGNN_OK;
  if (!gat_args_ok(src_index, dst_index, num_edge, el, er, feat, feat_ld, num_dst, num_head, num_feat, attn_p, ws,
                   ws_bytes))
    return FGNN_EINVAL;
  if (!alpha || !gout || gout_ld < num_head * num_feat || !fits_u32(gout_ld) ||
      (gfeat && (gfeat_ld < num_head * num_feat || !fits_u32(gfeat_ld))) || !float_aligned(alpha) ||
      !float_aligned(gout) || !float_aligned(gfeat) || !float_aligned(gel) || !float_aligned(ger) ||
      !float_aligned(d_step))
    return FGNN_EINVAL;
  if (!gfeat && !gel && !ger) return FGNN_OK;
  auto st = static_cast<hipStream_t>(stream);
  const GatWs w = gat_ws(ws, num_edge, num_dst, num_head);
  const uint32_t H = (uint32_t)num_head, F = (uint32_t)num_feat;
  const size_t total = num_edge * num_head, dim = num_head * num_feat;
  const unsigned edge_blocks = (unsigned)div_up(num_edge, (size_t)kBlock);
  const bool drop = attn_p > 0.f, scores = gel || ger;
  float *ga = w.sc;
  if (scores) {
    hipLaunchKernelGGL(gat_zero_kernel, dim3(capped_grid(num_dst * num_head)), dim3(kBlock), 0, st, w.t,
                       num_dst * num_head);
    if (F <= 64 && (F & (F - 1)) == 0) {
      const size_t blocks = div_up(div_up(num_edge, (size_t)kEdgesPerWave), (size_t)kWavesPerBlock);
      using Kernel = decltype(&gat_edge_dot_pow2_kernel<1>);
      static constexpr Kernel kernels[3] = {gat_edge_dot_pow2_kernel<1>, gat_edge_dot_pow2_kernel<2>,
                                            gat_edge_dot_pow2_kernel<4>};
      hipLaunchKernelGGL(kernels[dim <= 64 ? 0 : (dim <= 128 ? 1 : 2)], dim3(blocks), dim3(kBlock), 0, st, src_index,
                         dst_index, feat, gout, ga, num_edge, H, F, (uint32_t)dim, (uint32_t)feat_ld,
                         (uint32_t)gout_ld);
    } else {
      hipLaunchKernelGGL(gat_edge_dot_kernel, dim3(capped_grid(total)), dim3(kBlock), 0, st, src_index, dst_index, feat,
                         gout, ga, total, H, F, (uint32_t)feat_ld, (uint32_t)gout_ld);
    }
  }
  if (scores || (drop && gfeat))
    hipLaunchKernelGGL(gat_mask_t_kernel, dim3(edge_blocks), dim3(kBlock), 0, st, dst_index, num_edge, H, alpha,
                       scores ? ga : nullptr, drop ? w.aw : nullptr, w.t, attn_p, 1.0f / (1.0f - attn_p), seed, d_step,
                       tag);
  if (scores)
    hipLaunchKernelGGL(gat_score_grad_kernel, dim3(edge_blocks), dim3(kBlock), 0, st, src_index, dst_index, el, er,
                       num_edge, H, negative_slope, alpha, ga, w.t, gel, ger);
  if (gfeat)  // the forward's aggregation with the index arrays swapped: the mask is keyed by edge
    launch_gat_aggregate(dst_index, src_index, drop ? w.aw : alpha, gout, gout_ld, gfeat, gfeat_ld, num_edge, num_head,
                         num_feat, st);
  return launch_status(__func__);
}
