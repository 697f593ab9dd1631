// gatv2_attention.hip -- the attention aggregation of a GATv2 layer over a sampled block (examples/models.py:
// FusedGATv2Conv; the layer: dgl.nn.GATv2Conv).  H heads of F features, D = H F, fs [num_src, H, F], fd [num_dst, H, F]:
//     s[e,h] = sum_f attn[h,f] leaky_relu(fs[row[e],h,f] + fd[col[e],h,f])     a[e,h] = softmax of s over the edges of col[e]
//     out[col[e],h,:] += a~[e,h] fs[row[e],h,:]                                 a~ = a * keep / (1 - q)
// The score sits behind a per-element nonlinearity on an indexed pair of rows: op by op fs[row] + fd[col] (E x H x F) is
// materialised in both directions.  Here two kernels carry that work and nothing wider than E x H is written:
//   forward    zero m, z | SCORE + SEGMENT MAX | exp + segment sum | normalise (+ dropout mask) | aggregation of fs
//   backward   zero t | edge dot products ga = <g[col], fs[row]> | mask, t = sum a ga | gs = a (ga - t) |
//              FUSED GRADIENT PASS: gfs, gfd and gattn from one walk over the edges
// Every other pass is gat_common.h's (what gat_attention.hip runs).  Both kernels have block_aggregate_kernel's shape: a
// wave owns 32 edges and broadcasts their indices by shuffle, lane l owns columns l + 64 q of a trip of 64 P columns,
// the lane's attn slots and -- while the destination does not change -- its fd[col] (backward: gout[col] too) slots
// stay in registers, several fs[row] loads are in flight.  fp32; the order of the additions is not fixed.
#include "gat_common.h"

namespace fgnn {
namespace {

// Score + segment max.  The products attn * leaky_relu(fs + fd) of a head are reduced by xor shuffles over the R =
// min(F, 64) lanes that hold it in a slot: an aligned group for F a power of two <= 64, the whole wave for F a multiple
// of 64 (the launcher picks P so that a trip holds whole heads or a head whole trips).  The group's first lane puts the
// sum into the wave's own LDS stage [32 edges][heads of a trip] -- adds it, where a head has more than one slot -- and
// once a trip completes its heads the wave turns around: lane i reads edge i's scores from the stage, writes them to
// sc and takes part in the segmented max over the runs of equal destinations, one atomicMax per (wave, run, head).
// Only the owning wave touches its stage: no barrier, LDS operations of one wave complete in order.
template <int P>
__global__ __launch_bounds__(kBlock) void gatv2_score_max_kernel(const uint32_t *__restrict__ src_idx,
                                                                 const uint32_t *__restrict__ dst_idx,
                                                                 const float *__restrict__ fs,
                                                                 const float *__restrict__ fd,
                                                                 const float *__restrict__ attn, size_t num_edge,
                                                                 uint32_t H, uint32_t F, uint32_t dim, uint32_t fs_ld,
                                                                 uint32_t fd_ld, float slope, uint32_t stage_ld,
                                                                 float *__restrict__ sc, uint32_t *mkey) {
  extern __shared__ float stage_all[];
  const size_t wave = (size_t)blockIdx.x * kWavesPerBlock + wave_id();
  const size_t e0 = wave * kEdgesPerWave;
  if (e0 >= num_edge) return;  // wave-uniform
  const size_t e1 = e0 + kEdgesPerWave < num_edge ? e0 + kEdgesPerWave : num_edge;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t cnt = (uint32_t)(e1 - e0);
  const bool live = lane < cnt;
  uint32_t my_src = 0, my_dst = 0;
  if (live) {
    my_src = src_idx[e0 + lane];
    my_dst = dst_idx[e0 + lane];
  }
  const Runs r = wave_runs(my_dst, live, lane);
  float *stage = stage_all + (size_t)wave_id() * kEdgesPerWave * stage_ld;
  const uint32_t R = F < (uint32_t)kWave ? F : (uint32_t)kWave;
  const bool writer = (lane & (R - 1u)) == 0u;
  for (uint32_t dbase = 0; dbase < dim; dbase += kWave * P) {
    const uint32_t h0 = dbase / F;  // the stage's first head
    bool act[P], first[P];
    uint32_t slot[P];
    float av[P], fdv[P];
    uint32_t cur = __shfl(my_dst, 0, kWave);
    {
      const float *dp = fd + (size_t)cur * fd_ld + dbase + lane;
#pragma unroll
      for (int q = 0; q < P; ++q) {
        const uint32_t c = dbase + lane + kWave * q;
        act[q] = c < dim;
        slot[q] = act[q] ? c / F - h0 : 0u;
        first[q] = c % F == 0u;
        av[q] = act[q] ? attn[c] : 0.0f;
        fdv[q] = act[q] ? dp[kWave * q] : 0.0f;
      }
    }
    constexpr uint32_t UN = 4;  // edges whose fs rows are in flight together
    for (uint32_t i0 = 0; i0 < cnt; i0 += UN) {
      float v[UN][P];
      uint32_t c[UN];
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        const uint32_t i = i0 + u < cnt ? i0 + u : cnt - 1;  // clamp: the extra loads are discarded below
        const uint32_t sidx = __shfl(my_src, (int)i, kWave);
        c[u] = __shfl(my_dst, (int)i, kWave);
        const float *sp = fs + (size_t)sidx * fs_ld + dbase + lane;
#pragma unroll
        for (int q = 0; q < P; ++q) v[u][q] = act[q] ? sp[kWave * q] : 0.0f;
      }
#pragma unroll
      for (uint32_t u = 0; u < UN; ++u) {
        if (i0 + u >= cnt) break;  // wave-uniform
        if (c[u] != cur) {         // wave-uniform: another destination, another fd row
          cur = c[u];
          const float *dp = fd + (size_t)cur * fd_ld + dbase + lane;
#pragma unroll
          for (int q = 0; q < P; ++q) fdv[q] = act[q] ? dp[kWave * q] : 0.0f;
        }
        float *srow = stage + (size_t)(i0 + u) * stage_ld;
#pragma unroll
        for (int q = 0; q < P; ++q) {
          const float x = v[u][q] + fdv[q];
          float s = av[q] * (x > 0.0f ? x : slope * x);
          for (uint32_t d = R >> 1; d > 0; d >>= 1) s += __shfl_xor(s, (int)d, kWave);  // wave-uniform trip count
          if (writer && act[q]) srow[slot[q]] = first[q] ? s : srow[slot[q]] + s;
        }
      }
    }
    const uint32_t done = dbase + kWave * P;
    if (done >= dim || done % F == 0u) {  // wave-uniform: the heads h0 .. hend - 1 are complete
      const uint32_t hend = done >= dim ? H : done / F;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (uint32_t h = h0; h < hend; ++h) {
        float s = -__builtin_inff();
        if (live) {
          s = stage[(size_t)lane * stage_ld + (h - h0)];
          sc[(e0 + lane) * H + h] = s;
        }
        const float m = run_max(s, r.first, lane);
        if (r.tail) atomicMax(&mkey[(size_t)my_dst * H + h], float_key(m));
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

// every other F, pass 1 of 2: one thread per (edge, head) walks the head's F columns of both rows
__global__ __launch_bounds__(kBlock) void gatv2_score_kernel(const uint32_t *__restrict__ src_idx,
                                                             const uint32_t *__restrict__ dst_idx,
                                                             const float *__restrict__ fs,
                                                             const float *__restrict__ fd,
                                                             const float *__restrict__ attn, size_t total, uint32_t H,
                                                             uint32_t F, uint32_t fs_ld, uint32_t fd_ld, float slope,
                                                             float *__restrict__ sc) {
  for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kBlock) {
    const size_t e = idx / H;
    const uint32_t h = (uint32_t)(idx - e * H);
    const float *sp = fs + (size_t)src_idx[e] * fs_ld + (size_t)h * F;
    const float *dp = fd + (size_t)dst_idx[e] * fd_ld + (size_t)h * F;
    const float *ap = attn + (size_t)h * F;
    float s = 0.0f;
    for (uint32_t f = 0; f < F; ++f) {
      const float x = sp[f] + dp[f];
      s += ap[f] * (x > 0.0f ? x : slope * x);
    }
    sc[idx] = s;
  }
}

// pass 2 of 2: the segment max over scores that are in sc already (one lane per edge, gat_score_max_kernel's shape)
__global__ __launch_bounds__(kBlock) void gatv2_segment_max_kernel(const uint32_t *__restrict__ dst_idx,
                                                                   size_t num_edge, uint32_t H,
                                                                   const float *__restrict__ sc, uint32_t *mkey) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = (uint32_t)lane_id();
  const bool live = e < num_edge;
  if (__ballot(live) == 0ull) return;  // wave-uniform
  const uint32_t col = live ? dst_idx[e] : 0u;
  const Runs r = wave_runs(col, live, lane);
  for (uint32_t h = 0; h < H; ++h) {
    const float m = run_max(live ? sc[e * H + h] : -__builtin_inff(), r.first, lane);
    if (r.tail) atomicMax(&mkey[(size_t)col * H + h], float_key(m));
  }
}

// the score-gradient pass that stops at gs: ga[e,h] <- gs[e,h] = alpha (ga - t[col]), in place
__global__ __launch_bounds__(kBlock) void gatv2_gs_kernel(const uint32_t *__restrict__ dst_idx, size_t total, uint32_t H,
                                                          const float *__restrict__ alpha, const double *__restrict__ t,
                                                          float *__restrict__ ga) {
  for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kBlock) {
    const size_t e = idx / H;
    const uint32_t h = (uint32_t)(idx - e * H);
    ga[idx] = alpha[idx] * (ga[idx] - (float)t[(size_t)dst_idx[e] * H + h]);
  }
}

// Fused gradient pass: fs[row], fd[col] and gout[col] are read once each, u = fs + fd is recomputed, and with
// w = gs[e,h] attn[c] lrelu'(u):
//     gfs[row[e],c] += w + a~[e,h] gout[col[e],c]      one atomic per (edge, column): source rows do not repeat
//     gfd[col[e],c] += w                               summed in registers over a run of equal destinations
//     gattn[c]      += gs[e,h] lrelu(u)                summed in registers over ALL edges the wave walks
// The grid is bounded and a wave strides over the 32-edge chunks, so the number of gattn partial sums does not grow with
// E; a workgroup's four partial sums meet in LDS and leave as one atomic per (workgroup, column).  gattn is ONE small
// tensor that every edge adds to: its sums are kept in double from the chunk up (a chunk's 32 terms in fp32) and the
// workgroups' atomics go to a double scratch (gattn_acc, zeroed by the caller) that gatv2_gattn_add_kernel rounds into
// gattn once -- fp32 atomics on gattn itself (gattn_acc == null: no room in the workspace) round at the running sum's
// magnitude once per workgroup, in an order that changes from run to run.  Any F: nothing is reduced over a head's
// columns here.  Each output may be null (kernel-uniform).
template <int P>
__global__ __launch_bounds__(kBlock) void gatv2_grad_kernel(const uint32_t *__restrict__ src_idx,
                                                            const uint32_t *__restrict__ dst_idx,
                                                            const float *__restrict__ fs, const float *__restrict__ fd,
                                                            const float *__restrict__ attn,
                                                            const float *__restrict__ gout,
                                                            const float *__restrict__ gs, const float *__restrict__ aw,
                                                            size_t num_edge, uint32_t H, uint32_t F, uint32_t dim,
                                                            uint32_t fs_ld, uint32_t fd_ld, uint32_t gout_ld,
                                                            float slope, float *gfs, uint32_t gfs_ld, float *gfd,
                                                            uint32_t gfd_ld, float *gattn, double *gattn_acc) {
  __shared__ double red[kWavesPerBlock][kWave * P];
  const uint32_t lane = (uint32_t)lane_id();
  const size_t num_chunk = (num_edge + kEdgesPerWave - 1) / kEdgesPerWave;
  const size_t wave_stride = (size_t)gridDim.x * kWavesPerBlock;
  for (uint32_t dbase = 0; dbase < dim; dbase += kWave * P) {  // the same trips for every wave of the workgroup
    bool act[P];
    uint32_t head[P];
    float av[P];
    double gat_acc[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const uint32_t c = dbase + lane + kWave * q;
      act[q] = c < dim;
      head[q] = act[q] ? c / F : 0u;
      av[q] = act[q] ? attn[c] : 0.0f;
      gat_acc[q] = 0.0;
    }
    for (size_t chunk = (size_t)blockIdx.x * kWavesPerBlock + wave_id(); chunk < num_chunk; chunk += wave_stride) {
      const size_t e0 = chunk * kEdgesPerWave;
      const size_t e1 = e0 + kEdgesPerWave < num_edge ? e0 + kEdgesPerWave : num_edge;
      const uint32_t cnt = (uint32_t)(e1 - e0);
      uint32_t my_src = 0, my_dst = 0;
      if (lane < cnt) {
        my_src = src_idx[e0 + lane];
        my_dst = dst_idx[e0 + lane];
      }
      const float *gs_chunk = gs + e0 * H, *aw_chunk = aw + e0 * H;
      uint32_t cur = __shfl(my_dst, 0, kWave);
      float fdv[P], gv[P], gfd_acc[P], gat_chunk[P];
      {
        const float *dp = fd + (size_t)cur * fd_ld + dbase + lane;
        const float *gp = gout + (size_t)cur * gout_ld + dbase + lane;
#pragma unroll
        for (int q = 0; q < P; ++q) {
          fdv[q] = act[q] ? dp[kWave * q] : 0.0f;
          gv[q] = act[q] ? gp[kWave * q] : 0.0f;
          gfd_acc[q] = 0.0f;
          gat_chunk[q] = 0.0f;
        }
      }
      constexpr uint32_t UN = 2;  // edges in flight: a row and two weights per slot each
      for (uint32_t i0 = 0; i0 < cnt; i0 += UN) {
        float v[UN][P], gsv[UN][P], awv[UN][P];
        uint32_t c[UN], s[UN];
#pragma unroll
        for (uint32_t u = 0; u < UN; ++u) {
          const uint32_t i = i0 + u < cnt ? i0 + u : cnt - 1;  // clamp: the extra loads are discarded below
          s[u] = __shfl(my_src, (int)i, kWave);
          c[u] = __shfl(my_dst, (int)i, kWave);
          const float *sp = fs + (size_t)s[u] * fs_ld + dbase + lane;
          const float *gsp = gs_chunk + (size_t)i * H, *awp = aw_chunk + (size_t)i * H;
#pragma unroll
          for (int q = 0; q < P; ++q) {
            v[u][q] = act[q] ? sp[kWave * q] : 0.0f;
            gsv[u][q] = act[q] ? gsp[head[q]] : 0.0f;
            awv[u][q] = act[q] && gfs ? awp[head[q]] : 0.0f;
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < UN; ++u) {
          if (i0 + u >= cnt) break;  // wave-uniform
          if (c[u] != cur) {         // wave-uniform: the run ends, its gfd sums leave, the next rows come in
            if (gfd) {
              float *op = gfd + (size_t)cur * gfd_ld + dbase + lane;
#pragma unroll
              for (int q = 0; q < P; ++q)
                if (act[q]) unsafeAtomicAdd(op + kWave * q, gfd_acc[q]);
            }
            cur = c[u];
            const float *dp = fd + (size_t)cur * fd_ld + dbase + lane;
            const float *gp = gout + (size_t)cur * gout_ld + dbase + lane;
#pragma unroll
            for (int q = 0; q < P; ++q) {
              fdv[q] = act[q] ? dp[kWave * q] : 0.0f;
              gv[q] = act[q] ? gp[kWave * q] : 0.0f;
              gfd_acc[q] = 0.0f;
            }
          }
          float *op = gfs ? gfs + (size_t)s[u] * gfs_ld + dbase + lane : nullptr;
#pragma unroll
          for (int q = 0; q < P; ++q) {
            const float x = v[u][q] + fdv[q];
            const bool pos = x > 0.0f;
            const float ga_ = gsv[u][q] * av[q];
            const float w = pos ? ga_ : slope * ga_;
            gat_chunk[q] += gsv[u][q] * (pos ? x : slope * x);
            gfd_acc[q] += w;
            if (gfs && act[q]) unsafeAtomicAdd(op + kWave * q, w + awv[u][q] * gv[q]);
          }
        }
      }
      if (gfd) {
        float *op = gfd + (size_t)cur * gfd_ld + dbase + lane;
#pragma unroll
        for (int q = 0; q < P; ++q)
          if (act[q]) unsafeAtomicAdd(op + kWave * q, gfd_acc[q]);
      }
#pragma unroll
      for (int q = 0; q < P; ++q) gat_acc[q] += (double)gat_chunk[q];  // 32 terms in fp32, the chunks in double
    }
    if (gattn) {  // kernel-uniform, and every wave of the workgroup makes every trip: the barriers are safe
#pragma unroll
      for (int q = 0; q < P; ++q) red[wave_id()][lane + kWave * q] = gat_acc[q];
      __syncthreads();
      for (uint32_t j = threadIdx.x; j < (uint32_t)(kWave * P); j += kBlock) {
        double sum = red[0][j];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) sum += red[w][j];
        if (dbase + j < dim) {
          if (gattn_acc) unsafeAtomicAdd(gattn_acc + dbase + j, sum);
          else unsafeAtomicAdd(gattn + dbase + j, (float)sum);
        }
      }
      __syncthreads();
    }
  }
}

// gattn[c] += the double sums of the gradient pass, one rounding per element
__global__ __launch_bounds__(kBlock) void gatv2_gattn_add_kernel(float *gattn, const double *__restrict__ acc,
                                                                 uint32_t dim) {
  for (uint32_t c = blockIdx.x * kBlock + threadIdx.x; c < dim; c += gridDim.x * kBlock) gattn[c] += (float)acc[c];
}

// ---- host side -------------------------------------------------------------------------------------------------------

// workspace: z | t as doubles, num_dst H each, then in floats m (encoded max), num_dst H; per-edge scores (then ga, then
// gs) | dropped-out weights, num_edge H each.  Double segment sums: a hub's z and t collect thousands of atomics, and at
// a small H F every edge's gattn term leans on them
struct Gatv2Ws {
  double *z, *t;
  uint32_t *mkey;
  float *sc, *aw;
};
inline size_t gatv2_ws_floats(size_t num_edge, size_t num_dst, size_t num_head) {
  return 5 * num_dst * num_head + 2 * num_edge * num_head;
}
inline Gatv2Ws gatv2_ws(void *ws, size_t num_edge, size_t num_dst, size_t num_head) {
  const size_t nd = num_dst * num_head, ne = num_edge * num_head;
  double *d = static_cast<double *>(ws);
  float *p = static_cast<float *>(ws) + 4 * nd;
  return Gatv2Ws{d, d + nd, reinterpret_cast<uint32_t *>(p), p + nd, p + nd + ne};
}

inline bool pow2_le_64(size_t F) { return F <= 64 && (F & (F - 1)) == 0; }

// Slots per lane of the score kernel: a trip of 64 P columns must hold whole heads or lie inside one head, and its
// heads -- the width of the LDS stage -- stay at 64 or fewer
inline int gatv2_score_slots(size_t F, size_t dim) {
  int p = 1;
  for (int cand = 4; cand > 1; cand >>= 1) {
    const size_t w = (size_t)kWave * cand;
    if ((w % F == 0 || F % w == 0) && w / F <= 64) {
      p = cand;
      break;
    }
  }
  const int by_dim = dim <= 64 ? 1 : (dim <= 128 ? 2 : 4);
  return p < by_dim ? p : by_dim;
}

// what both entry points refuse before any launch
bool gatv2_args_ok(const uint32_t *src_index, const uint32_t *dst_index, size_t num_edge, const float *fs, size_t fs_ld,
                   const float *fd, size_t fd_ld, const float *attn, size_t num_dst, size_t num_head, size_t num_feat,
                   float attn_p, const unsigned long long *d_step, const void *ws, size_t ws_bytes) {
  if (!src_index || !dst_index || !fs || !fd || !attn || !ws || num_head == 0 || num_feat == 0) return false;
  if (!fits_u32(num_head) || !fits_u32(num_feat) || !fits_u32(num_head * num_feat) || !fits_u32(num_dst) ||
      fs_ld < num_head * num_feat || !fits_u32(fs_ld) || fd_ld < num_head * num_feat || !fits_u32(fd_ld) ||
      !(attn_p >= 0.f && attn_p < 1.f))
    return false;
  if (!float_aligned(src_index) || !float_aligned(dst_index) || !float_aligned(fs) || !float_aligned(fd) ||
      !float_aligned(attn) || !float_aligned(d_step) || (reinterpret_cast<uintptr_t>(ws) & 7u) != 0)
    return false;
  if (ws_bytes < fgnn_gatv2_workspace_bytes(num_edge, num_dst, num_head)) return false;
  return edge_wave_blocks(num_edge) <= 0x7fffffffull;
}

}  // namespace
}  // namespace fgnn

extern "C" size_t fgnn_gatv2_workspace_bytes(size_t num_edge, size_t num_dst, size_t num_head) {
  return fgnn::gatv2_ws_floats(num_edge, num_dst, num_head) * sizeof(float);
}

extern "C" int fgnn_gatv2_forward(const uint32_t *src_index, const uint32_t *dst_index, size_t num_edge, const float *fs,
                                  size_t fs_ld, const float *fd, size_t fd_ld, const float *attn, size_t num_dst,
                                  size_t num_head, size_t num_feat, float negative_slope, float attn_p, uint64_t seed,
                                  const unsigned long long *d_step, uint32_t tag, float *alpha, float *out,
                                  size_t out_ld, void *ws, size_t ws_bytes, void *stream) {
  using namespace fgnn;
  if (num_edge == 0) return FGNN_OK;
  if (!gatv2_args_ok(src_index, dst_index, num_edge, fs, fs_ld, fd, fd_ld, attn, num_dst, num_head, num_feat, attn_p,
                     d_step, ws, ws_bytes))
    return FGNN_EINVAL;
  if (!alpha || !out || out_ld < num_head * num_feat || !fits_u32(out_ld) || !float_aligned(alpha) ||
      !float_aligned(out))
    return FGNN_EINVAL;
  auto st = static_cast<hipStream_t>(stream);
  const Gatv2Ws w = gatv2_ws(ws, num_edge, num_dst, num_head);
  const uint32_t H = (uint32_t)num_head, F = (uint32_t)num_feat;
  const size_t total = num_edge * num_head, dim = num_head * num_feat;
  const unsigned edge_blocks = (unsigned)div_up(num_edge, (size_t)kBlock);
  const bool drop = attn_p > 0.f;
  hipLaunchKernelGGL(gat_zero_kernel, dim3(capped_grid(5 * num_dst * num_head)), dim3(kBlock), 0, st,
                     reinterpret_cast<float *>(w.z), 5 * num_dst * num_head);  // z, (t,) m: one fill
  if (pow2_le_64(num_feat) || num_feat % 64 == 0) {
    const int p = gatv2_score_slots(num_feat, dim);
    const size_t trip = (size_t)kWave * p;
    const uint32_t stage_ld = (uint32_t)(trip > num_feat ? trip / num_feat : 1) | 1u;  // odd: no bank conflicts
    using Kernel = decltype(&gatv2_score_max_kernel<1>);
    static constexpr Kernel kernels[3] = {gatv2_score_max_kernel<1>, gatv2_score_max_kernel<2>,
                                          gatv2_score_max_kernel<4>};
    hipLaunchKernelGGL(kernels[p == 1 ? 0 : (p == 2 ? 1 : 2)], dim3(edge_wave_blocks(num_edge)), dim3(kBlock),
                       (size_t)kWavesPerBlock * kEdgesPerWave * stage_ld * sizeof(float), st, src_index, dst_index, fs,
                       fd, attn, num_edge, H, F, (uint32_t)dim, (uint32_t)fs_ld, (uint32_t)fd_ld, negative_slope,
                       stage_ld, w.sc, w.mkey);
  } else {
    hipLaunchKernelGGL(gatv2_score_kernel, dim3(capped_grid(total)), dim3(kBlock), 0, st, src_index, dst_index, fs, fd,
                       attn, total, H, F, (uint32_t)fs_ld, (uint32_t)fd_ld, negative_slope, w.sc);
    hipLaunchKernelGGL(gatv2_segment_max_kernel, dim3(edge_blocks), dim3(kBlock), 0, st, dst_index, num_edge, H, w.sc,
                       w.mkey);
  }
  hipLaunchKernelGGL(gat_exp_sum_kernel<double>, dim3(edge_blocks), dim3(kBlock), 0, st, dst_index, num_edge, H, w.sc, w.mkey,
                     w.z);
  hipLaunchKernelGGL(gat_normalise_kernel<double>, dim3(capped_grid(div_up(total, (size_t)4))), dim3(kBlock), 0, st, dst_index,
                     total, H, w.sc, w.z, alpha, drop ? w.aw : nullptr, attn_p, 1.0f / (1.0f - attn_p), seed, d_step,
                     tag);
  launch_gat_aggregate(src_index, dst_index, drop ? w.aw : alpha, fs, fs_ld, out, out_ld, num_edge, num_head, num_feat,
                       st);
  return launch_status(__func__);
}

extern "C" int fgnn_gatv2_backward(const uint32_t *src_index, const uint32_t *dst_index, size_t num_edge,
                                   const float *fs, size_t fs_ld, const float *fd, size_t fd_ld, const float *attn,
                                   const float *alpha, const float *gout, size_t gout_ld, size_t num_dst,
                                   size_t num_head, size_t num_feat, float negative_slope, float attn_p, uint64_t seed,
                                   const unsigned long long *d_step, uint32_t tag, float *gfs, size_t gfs_ld, float *gfd,
                                   size_t gfd_ld, float *gattn, void *ws, size_t ws_bytes, void *stream) {
  using namespace fgnn;
  if (num_edge == 0) return FGNN_OK;
  if (!gatv2_args_ok(src_index, dst_index, num_edge, fs, fs_ld, fd, fd_ld, attn, num_dst, num_head, num_feat, attn_p,
                     d_step, ws, ws_bytes))
    return FGNN_EINVAL;
  const size_t dim = num_head * num_feat;
  if (!alpha || !gout || gout_ld < dim || !fits_u32(gout_ld) || (gfs && (gfs_ld < dim || !fits_u32(gfs_ld))) ||
      (gfd && (gfd_ld < dim || !fits_u32(gfd_ld))) || !float_aligned(alpha) || !float_aligned(gout) ||
      !float_aligned(gfs) || !float_aligned(gfd) || !float_aligned(gattn))
    return FGNN_EINVAL;
  if (!gfs && !gfd && !gattn) return FGNN_OK;
  auto st = static_cast<hipStream_t>(stream);
  const Gatv2Ws w = gatv2_ws(ws, num_edge, num_dst, num_head);
  const uint32_t H = (uint32_t)num_head, F = (uint32_t)num_feat;
  const size_t total = num_edge * num_head;
  const unsigned edge_blocks = (unsigned)div_up(num_edge, (size_t)kBlock);
  const bool drop = attn_p > 0.f;
  float *ga = w.sc;
  // the backward pass has no use for z: its num_dst H doubles hold gattn's H F sums where they fit (num_dst >= F);
  // zeroed with t, which follows it
  double *gattn_acc = gattn && num_dst >= num_feat ? w.z : nullptr;
  hipLaunchKernelGGL(gat_zero_kernel, dim3(capped_grid(4 * num_dst * num_head)), dim3(kBlock), 0, st,
                     reinterpret_cast<float *>(w.z), 4 * num_dst * num_head);
  launch_gat_edge_dot(src_index, dst_index, fs, fs_ld, gout, gout_ld, ga, num_edge, num_head, num_feat, st);
  hipLaunchKernelGGL(gat_mask_t_kernel<double>, dim3(edge_blocks), dim3(kBlock), 0, st, dst_index, num_edge, H, alpha, ga,
                     drop ? w.aw : nullptr, w.t, attn_p, 1.0f / (1.0f - attn_p), seed, d_step, tag);
  hipLaunchKernelGGL(gatv2_gs_kernel, dim3(capped_grid(total)), dim3(kBlock), 0, st, dst_index, total, H, alpha, w.t,
                     ga);
  // four workgroups per CU at most: the gattn partial sums -- one atomic per (workgroup, column) -- stay bounded
  const size_t want = edge_wave_blocks(num_edge), cap = (size_t)device_cu_count() * 4;
  using Kernel = decltype(&gatv2_grad_kernel<1>);
  static constexpr Kernel kernels[3] = {gatv2_grad_kernel<1>, gatv2_grad_kernel<2>, gatv2_grad_kernel<4>};
  hipLaunchKernelGGL(kernels[dim <= 64 ? 0 : (dim <= 128 ? 1 : 2)], dim3(want < cap ? want : cap), dim3(kBlock), 0, st,
                     src_index, dst_index, fs, fd, attn, gout, ga, drop ? w.aw : alpha, num_edge, H, F, (uint32_t)dim,
                     (uint32_t)fs_ld, (uint32_t)fd_ld, (uint32_t)gout_ld, negative_slope, gfs, (uint32_t)gfs_ld, gfd,
                     (uint32_t)gfd_ld, gattn, gattn_acc);
  if (gattn_acc)
    hipLaunchKernelGGL(gatv2_gattn_add_kernel, dim3(capped_grid(dim)), dim3(kBlock), 0, st, gattn, gattn_acc,
                       (uint32_t)dim);
  return launch_status(__func__);
}
