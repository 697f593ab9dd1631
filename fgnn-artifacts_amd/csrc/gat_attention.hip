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
// Everything but the two score passes below lives in gat_common.h, which gatv2_attention.hip shares.
#include "gat_common.h"

namespace fgnn {
namespace {

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
  hipLaunchKernelGGL(gat_exp_sum_kernel<float>, dim3(edge_blocks), dim3(kBlock), 0, st, dst_index, num_edge, H, w.sc, w.mkey,
                     w.z);
  hipLaunchKernelGGL(gat_normalise_kernel<float>, dim3(capped_grid(div_up(total, (size_t)4))), dim3(kBlock), 0, st, dst_index,
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
  const uint32_t H = (uint32_t)num_head;
  const unsigned edge_blocks = (unsigned)div_up(num_edge, (size_t)kBlock);
  const bool drop = attn_p > 0.f, scores = gel || ger;
  float *ga = w.sc;
  if (scores) {
    hipLaunchKernelGGL(gat_zero_kernel, dim3(capped_grid(num_dst * num_head)), dim3(kBlock), 0, st, w.t,
                       num_dst * num_head);
    launch_gat_edge_dot(src_index, dst_index, feat, feat_ld, gout, gout_ld, ga, num_edge, num_head, num_feat, st);
  }
  if (scores || (drop && gfeat))
    hipLaunchKernelGGL(gat_mask_t_kernel<float>, dim3(edge_blocks), dim3(kBlock), 0, st, dst_index, num_edge, H, alpha,
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
