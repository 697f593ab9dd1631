// gat_common.h -- what the attention layers over a sampled block share (gat_attention.hip: GAT, gatv2_attention.hip:
// GATv2): the monotone float key of the segment max, the runs of equal destinations over a wave, the Philox keep rule,
// and every pass behind the score -- exp + segment sum, normalise (+ dropout mask), the weighted aggregation, the edge
// dot products, mask + t -- with the workspace they work in.  Each translation unit gets its own copy of the kernels.
#pragma once
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

// The segment sums z and t are float (GAT) or double (GATv2: A = double makes them independent of the order in which the
// atomics land, up to 2^-53) -- the kernels below take the accumulator type as a parameter and round to float on use.

// pass 2: sc[e,h] = exp(sc[e,h] - m[col,h]); z[col,h] += it
template <typename A>
__global__ __launch_bounds__(kBlock) void gat_exp_sum_kernel(const uint32_t *__restrict__ dst_idx, size_t num_edge,
                                                             uint32_t H, float *__restrict__ sc,
                                                             const uint32_t *__restrict__ mkey, A *z) {
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
    if (r.tail) unsafeAtomicAdd(&z[(size_t)col * H + h], (A)s);
  }
}

// pass 3: alpha = p / z[col]; aw = alpha * keep / (1 - q) when a mask is drawn (aw == null: none).  A thread takes
// the four elements of one Philox block; E H need not be a multiple of 4.
template <typename A>
__global__ __launch_bounds__(kBlock) void gat_normalise_kernel(const uint32_t *__restrict__ dst_idx, size_t total,
                                                               uint32_t H, const float *__restrict__ sc,
                                                               const A *__restrict__ z, float *__restrict__ alpha,
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
      const float a = sc[idx] / (float)z[(size_t)dst_idx[e] * H + h];
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
template <typename A>
__global__ __launch_bounds__(kBlock) void gat_mask_t_kernel(const uint32_t *__restrict__ dst_idx, size_t num_edge,
                                                            uint32_t H, const float *__restrict__ alpha, float *ga,
                                                            float *__restrict__ aw, A *t, float p, float scale,
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
      if (r.tail) unsafeAtomicAdd(&t[(size_t)col * H + h], (A)s);
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

// workgroups of a kernel in which a wave owns 32 edges
inline size_t edge_wave_blocks(size_t num_edge) {
  return div_up(div_up(num_edge, (size_t)kEdgesPerWave), (size_t)kWavesPerBlock);
}

inline void launch_gat_aggregate(const uint32_t *src_index, const uint32_t *dst_index, const float *wgt, const float *h,
                                 size_t h_ld, float *out, size_t out_ld, size_t num_edge, size_t H, size_t F,
                                 hipStream_t st) {
  const size_t dim = H * F;
  using Kernel = decltype(&gat_aggregate_kernel<1>);
  static constexpr Kernel kernels[3] = {gat_aggregate_kernel<1>, gat_aggregate_kernel<2>, gat_aggregate_kernel<4>};
  hipLaunchKernelGGL(kernels[dim <= 64 ? 0 : (dim <= 128 ? 1 : 2)], dim3(edge_wave_blocks(num_edge)), dim3(kBlock), 0,
                     st, src_index, dst_index, wgt, h, out, num_edge, (uint32_t)H, (uint32_t)F, (uint32_t)dim,
                     (uint32_t)h_ld, (uint32_t)out_ld);
}

// ga[e,h] = <g[dst_index[e],h,:], feat[src_index[e],h,:]>
inline void launch_gat_edge_dot(const uint32_t *src_index, const uint32_t *dst_index, const float *feat, size_t feat_ld,
                                const float *g, size_t g_ld, float *ga, size_t num_edge, size_t num_head,
                                size_t num_feat, hipStream_t st) {
  const uint32_t H = (uint32_t)num_head, F = (uint32_t)num_feat;
  const size_t total = num_edge * num_head, dim = num_head * num_feat;
  if (F <= 64 && (F & (F - 1)) == 0) {
    using Kernel = decltype(&gat_edge_dot_pow2_kernel<1>);
    static constexpr Kernel kernels[3] = {gat_edge_dot_pow2_kernel<1>, gat_edge_dot_pow2_kernel<2>,
                                          gat_edge_dot_pow2_kernel<4>};
    hipLaunchKernelGGL(kernels[dim <= 64 ? 0 : (dim <= 128 ? 1 : 2)], dim3(edge_wave_blocks(num_edge)), dim3(kBlock), 0,
                       st, src_index, dst_index, feat, g, ga, num_edge, H, F, (uint32_t)dim, (uint32_t)feat_ld,
                       (uint32_t)g_ld);
  } else {
    hipLaunchKernelGGL(gat_edge_dot_kernel, dim3(capped_grid(total)), dim3(kBlock), 0, st, src_index, dst_index, feat,
                       g, ga, total, H, F, (uint32_t)feat_ld, (uint32_t)g_ld);
  }
}

}  // namespace
}  // namespace fgnn
