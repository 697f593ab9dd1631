"""GNN layers on the COO blocks the engine returns, written with plain torch ops (DGL has no ROCm wheel in this image;
with DGL installed `get_dgl_blocks` returns DGLBlocks and the dgl.nn layers work unchanged).

Block convention (samgraph/torch/adapter.py): row[e] = local id of the sampled neighbour (source), col[e] = local id
of the seed (destination); the first number_of_dst_nodes() source nodes are the destination nodes themselves."""
import os

import torch as th
import torch.nn as nn
import torch.nn.functional as F

try:  # fused gather + segment-sum kernel of this repo (fgnn_hip/nn.py); FGNN_TORCH_AGGREGATE=1 forces the torch ops
    from fgnn_hip.nn import block_aggregate as _fused_aggregate
except ImportError:
    _fused_aggregate = None
if os.environ.get("FGNN_TORCH_AGGREGATE"):
    _fused_aggregate = None


# The weight gradient of a layer, gw = gy^T z, reduces over the rows (tens of thousands of nodes) into a small matrix:
# a handful of output tiles, so the library GEMM runs at a fraction of the chip unless the reduction is split -- a
# batched GEMM over s row slices followed by a sum.  Which s wins is erratic (MI355X, fp32, tools/gw_microbench.py:
# 22 500 x 256 x 256: library 111 us, s = 8 55 us, s = 32 181 us; 8 000 x 256 x 256: library 49 us, s = 8 231 us), so
# the first call of a shape times the candidates once and the choice is kept per (rows / 2048, widths).
_GW_CHOICE = {}


def _gw_slices(gy, z, s):
    m = gy.shape[0]
    mp = (m // s) * s
    gw = th.bmm(gy[:mp].view(s, mp // s, -1).transpose(1, 2), z[:mp].view(s, mp // s, -1)).sum(0)
    return gw + gy[mp:].t().mm(z[mp:]) if mp < m else gw


def _weight_grad(gy, z):
    m = gy.shape[0]
    if not gy.is_cuda or m < 4096 or not (gy.is_contiguous() and z.is_contiguous()):
        return gy.t().mm(z)
    key = (m >> 11, gy.shape[1], z.shape[1], gy.dtype)
    s = _GW_CHOICE.get(key)
    if s is None and th.cuda.is_current_stream_capturing():
        s = 0  # no timing inside a capture: the library GEMM (eager steps before the capture have usually chosen already)
    if s is None:
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        best = (float("inf"), 0)
        for cand in (0, 8, 16, 64):
            fn = (lambda: gy.t().mm(z)) if cand == 0 else (lambda: _gw_slices(gy, z, cand))
            fn()
            e0.record()
            for _ in range(3):
                fn()
            e1.record()
            e1.synchronize()
            best = min(best, (e0.elapsed_time(e1), cand))
        s = _GW_CHOICE[key] = best[1]
    return _gw_slices(gy, z, s) if s else gy.t().mm(z)


class _TallLinearFn(th.autograd.Function):
    """y = x W^T + b for x with very many rows (10^5 nodes x 10^2 features); the weight gradient through _weight_grad."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        y = x.mm(weight.t())
        return y + bias if bias is not None else y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gy.mm(weight) if ctx.needs_input_grad[0] else None
        gw = _weight_grad(gy, x.contiguous())
        gb = gy.sum(0) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


class TallLinear(nn.Linear):
    def forward(self, x):
        if x.dim() == 2 and x.is_cuda and x.dtype == th.float32:
            return _TallLinearFn.apply(x, self.weight, self.bias)
        return super().forward(x)


def _fused_layers_apply(block, h):
    """the one rule for every layer here: the HIP path for fp32 CUDA features and int32 COO indices with the library
    present, the op-by-op arithmetic otherwise"""
    return (_fused_aggregate is not None and h.is_cuda and h.dtype == th.float32
            and getattr(block.row, "dtype", None) == th.int32 and block.col.dtype == th.int32)


def _half_rows_apply(block, h):
    """fp16 input features (the engine's `feat_store_dtype = f16`) that the first layer of the fused SAGE, GCN and
    PinSAGE models reads as they are: the aggregation kernels upcast the rows on load (fgnn_block_aggregate_ex_f16 /
    _scaled_f16, fgnn_sage_finish_z_f16), sums and everything behind them are fp32, and no fp32 copy of the num_src x D
    feature tensor is written.  Input features take no gradient."""
    return (_fused_aggregate is not None and h.is_cuda and h.dtype == th.float16 and not h.requires_grad
            and getattr(block.row, "dtype", None) == th.int32 and block.col.dtype == th.int32)


def input_rows(layer, block, x):
    """what a model hands its first layer: x itself -- unless x is fp16 and the layer cannot read half rows (GAT, every
    op-by-op layer, any layer off the GPU or without the HIP library): those get ONE torch upcast of the whole tensor,
    num_src x D, which is what a half-precision store otherwise saves"""
    if x.dtype != th.float16:
        return x
    if isinstance(layer, (FusedSAGEConv, FusedGraphConv, FusedWeightedSAGEConv)) and _half_rows_apply(block, x):
        return x
    return x.float()


def _sum_to_dst(block, h, weight=None):
    num_dst = block.number_of_dst_nodes()
    if _fused_layers_apply(block, h):
        return _fused_aggregate(h, block.row, block.col, num_dst, weight)
    row, col = block.row.long(), block.col.long()
    msg = h[row] if weight is None else h[row] * weight.unsqueeze(1)
    return th.zeros((num_dst, h.shape[1]), dtype=h.dtype, device=h.device).index_add_(0, col, msg)


def _in_degree(block, dtype, weight=None):
    num_dst = block.number_of_dst_nodes()
    col = block.col.long()
    ones = th.ones_like(col, dtype=dtype) if weight is None else weight
    return th.zeros(num_dst, dtype=dtype, device=col.device).index_add_(0, col, ones)


class SAGEConvMean(nn.Module):
    """h_dst' = W_self h_dst + W_neigh mean_{(u->v)} h_u   (dgl.nn.SAGEConv(..., 'mean'))"""

    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.fc_self = TallLinear(in_feats, out_feats, bias=False)
        self.fc_neigh = TallLinear(in_feats, out_feats, bias=True)

    def forward(self, block, h):
        num_dst = block.number_of_dst_nodes()
        agg = _sum_to_dst(block, h) / _in_degree(block, h.dtype).clamp(min=1).unsqueeze(1)
        return self.fc_self(h[:num_dst]) + self.fc_neigh(agg)


class _FusedSageFn(th.autograd.Function):
    """SAGEConv('mean') as ONE autograd node: z = [h_dst | mean_{(u->v)} h_u], out = z W^T + b with W = [W_self |
    W_neigh].  One GEMM forward instead of two, two backward instead of four; the neighbour sums land straight in the
    right half of z, the in-degrees are counted by the same launch (once per block), and there is no autograd
    bookkeeping for the dozen small ops in between -- a training step is bound by the number of ops Python launches,
    not by their GPU time (profiles/r04_c_train_*).  Same arithmetic as SAGEConvMean (fp32; the float additions of the
    GEMM are grouped differently: rtol 1e-4)."""

    @staticmethod
    def forward(ctx, h, weight, bias, block, num_dst):
        from fgnn_hip.nn import aggregate_into, sage_finish_z
        h = h.contiguous()
        din = h.shape[1]
        # z and the in-degree counts out of ONE zeroed buffer (one fill), the neighbour sums and the counts by one
        # launch, the mean's scaling and the copy of the destinations' own rows by one more (fgnn_sage_finish_z)
        buf = th.zeros(num_dst * (2 * din + 1), dtype=th.float32, device=h.device)  # (h may be fp16: upcast on load)
        z = buf[:num_dst * 2 * din].view(num_dst, 2 * din)
        deg = buf[num_dst * 2 * din:]
        aggregate_into(z[:, din:], h, block.row, block.col, in_degree=deg)
        if din % 4 == 0:
            inv = sage_finish_z(z, h, deg, num_dst, din)
        else:
            inv = deg.clamp(min=1).reciprocal_()
            z[:, din:] *= inv.unsqueeze(1)
            z[:, :din] = h[:num_dst]
        ctx.save_for_backward(z, weight, block.row, block.col, inv)
        ctx.num_src = h.shape[0]
        return th.addmm(bias, z, weight.t())

    @staticmethod
    def backward(ctx, gout):
        from fgnn_hip.nn import aggregate_into, sage_grad_prep
        z, weight, row, col, inv_deg = ctx.saved_tensors
        gout = gout.contiguous()
        din = z.shape[1] // 2
        gw = _weight_grad(gout, z) if ctx.needs_input_grad[1] else None
        gb = gout.sum(0) if ctx.needs_input_grad[2] else None
        gh = None
        if ctx.needs_input_grad[0]:
            gz = gout.mm(weight)
            if din % 4 == 0:  # self path + zero rows + scaled neighbour gradients in one launch
                gh, gagg = sage_grad_prep(gz, inv_deg, ctx.num_src, din)
                aggregate_into(gh, gagg, col, row)
            else:
                gagg = gz[:, din:] * inv_deg.unsqueeze(1)  # (contiguous: a new tensor)
                gh = aggregate_into(th.zeros((ctx.num_src, din), dtype=gz.dtype, device=gz.device), gagg, col, row)
                gh[:z.shape[0]] += gz[:, :din]
        return gh, gw, gb, None, None


class FusedSAGEConv(nn.Module):
    """SAGEConvMean with the layer's two linear maps as one weight [out, 2 in] = [W_self | W_neigh] and the whole layer
    as one autograd node (_FusedSageFn); falls back to the op-by-op formulation off the GPU / without the HIP
    library."""

    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.in_feats = in_feats
        self.weight = nn.Parameter(th.empty(out_feats, 2 * in_feats))
        self.bias = nn.Parameter(th.zeros(out_feats))
        for half in (self.weight[:, :in_feats], self.weight[:, in_feats:]):  # each map initialised like nn.Linear's
            nn.init.kaiming_uniform_(half, a=5 ** 0.5)
        bound = 1 / in_feats ** 0.5
        nn.init.uniform_(self.bias, -bound, bound)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """accepts the op-by-op layout too (fc_self.weight / fc_neigh.weight / fc_neigh.bias: SAGEConvMean here, DGL's
        SAGEConv in the reference's checkpoints): the two maps side by side are this layer's weight"""
        ks, kn, kb = prefix + "fc_self.weight", prefix + "fc_neigh.weight", prefix + "fc_neigh.bias"
        ksb = prefix + "fc_self.bias"
        if ks in state_dict and kn in state_dict and prefix + "weight" not in state_dict:
            state_dict[prefix + "weight"] = th.cat([state_dict.pop(ks), state_dict.pop(kn)], 1)
            # DGL < 0.8 keeps a bias in BOTH maps (their sum is what the layer adds); DGL >= 0.8 a separate `bias`
            # (already under this layer's name); SAGEConvMean here: fc_neigh.bias only
            parts = [state_dict.pop(k) for k in (kb, ksb) if k in state_dict]
            if parts and prefix + "bias" not in state_dict:
                state_dict[prefix + "bias"] = parts[0] if len(parts) == 1 else parts[0] + parts[1]
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def split_state_dict(self, prefix=""):
        """this layer's parameters in the op-by-op layout (what SAGEConvMean / DGL's SAGEConv load)"""
        d = self.in_feats
        return {prefix + "fc_self.weight": self.weight.detach()[:, :d].clone(),
                prefix + "fc_neigh.weight": self.weight.detach()[:, d:].clone(),
                prefix + "fc_neigh.bias": self.bias.detach().clone()}

    def forward(self, block, h):
        num_dst = block.number_of_dst_nodes()
        if _fused_layers_apply(block, h) or _half_rows_apply(block, h):
            return _FusedSageFn.apply(h, self.weight, self.bias, block, num_dst)
        agg = _sum_to_dst(block, h) / _in_degree(block, h.dtype).clamp(min=1).unsqueeze(1)
        return th.cat([h[:num_dst], agg], 1).mm(self.weight.t()) + self.bias


class GraphConv(nn.Module):
    """dgl.nn.GraphConv(norm='both', allow_zero_in_degree=True) as the reference's GCN uses it
    (example/samgraph/multi_gpu/train_gcn.py:24-47): D_out^-1/2 on the sources, D_in^-1/2 on the destinations."""

    def __init__(self, in_feats, out_feats, activation=None):
        super().__init__()
        self.fc = TallLinear(in_feats, out_feats, bias=True)
        self.activation = activation

    def conv(self, block, h):
        """the layer before its activation"""
        row = block.row.long()
        out_deg = th.zeros(h.shape[0], dtype=h.dtype, device=h.device).index_add_(
            0, row, th.ones_like(row, dtype=h.dtype)).clamp(min=1)
        h = h * out_deg.pow(-0.5).unsqueeze(1)
        agg = _sum_to_dst(block, h) * _in_degree(block, h.dtype).clamp(min=1).pow(-0.5).unsqueeze(1)
        return self.fc(agg)

    def forward(self, block, h, activate=True):
        """activate=False returns the pre-activation (the caller fuses the ReLU with its dropout)"""
        out = self.conv(block, h)
        return self.activation(out) if self.activation and activate else out


class WeightedSAGEConv(nn.Module):
    """PinSAGE's weighted aggregator (example/samgraph/multi_gpu/train_pinsage.py:24-75): neighbours weighted by
    their random-walk visit counts (block.edata['weights']), concatenated with the destination's own state."""

    def __init__(self, in_feats, hidden, out_feats, dropout):
        super().__init__()
        self.Q = TallLinear(in_feats, hidden)
        self.W = TallLinear(in_feats + hidden, out_feats)
        self.dropout = nn.Dropout(dropout)

    def forward(self, block, h):
        num_dst = block.number_of_dst_nodes()
        w = block.edata["weights"].to(h.dtype)
        n = _sum_to_dst(block, F.relu(self.Q(self.dropout(h))), w)
        ws = _in_degree(block, h.dtype, w).clamp(min=1).unsqueeze(1)
        z = F.relu(self.W(self.dropout(th.cat([n / ws, h[:num_dst]], 1))))
        z_norm = z.norm(2, 1, keepdim=True)
        return z / th.where(z_norm == 0, th.ones_like(z_norm), z_norm)


class _FusedGraphConvFn(th.autograd.Function):
    """GraphConv(norm='both') as ONE autograd node: both degree vectors from one pass over the edges
    (fgnn_block_degrees), D_out^-1/2 and D_in^-1/2 inside the aggregation (fgnn_block_aggregate_scaled: the source
    factor folded into the edge weight, the destination factor applied at the flush), then one GEMM with bias.  No
    scaled copy of h -- num_src x D, the largest tensor of the step -- is written, kept alive for the backward pass or
    read back by it; the input gradient is the same launch with the indices, degree vectors and modes swapped.  Same
    arithmetic as GraphConv (fp32; the order of the float additions differs: rtol 1e-4)."""

    @staticmethod
    def forward(ctx, h, weight, bias, block, num_dst):
        from fgnn_hip.nn import aggregate_scaled_into, block_degrees
        h = h.contiguous()
        src_deg, dst_deg = block_degrees(block.row, block.col, h.shape[0], num_dst)
        agg = th.zeros((num_dst, h.shape[1]), dtype=th.float32, device=h.device)  # (h may be fp16: upcast on load)
        aggregate_scaled_into(agg, h, block.row, block.col, None, src_deg, 1, dst_deg, 1)
        ctx.save_for_backward(agg, weight, block.row, block.col, src_deg, dst_deg)
        ctx.num_src = h.shape[0]
        return th.addmm(bias, agg, weight.t())

    @staticmethod
    def backward(ctx, gout):
        from fgnn_hip.nn import aggregate_scaled_into
        agg, weight, row, col, src_deg, dst_deg = ctx.saved_tensors
        gout = gout.contiguous()
        gw = _weight_grad(gout, agg) if ctx.needs_input_grad[1] else None
        gb = gout.sum(0) if ctx.needs_input_grad[2] else None
        gh = None
        if ctx.needs_input_grad[0]:
            gagg = gout.mm(weight)
            gh = th.zeros((ctx.num_src, agg.shape[1]), dtype=gagg.dtype, device=gagg.device)
            aggregate_scaled_into(gh, gagg, col, row, None, dst_deg, 1, src_deg, 1)
        return gh, gw, gb, None, None


class FusedGraphConv(GraphConv):
    """GraphConv with the whole layer as one autograd node (_FusedGraphConvFn); the same parameters under the same
    names (fc.weight, fc.bias), so state dicts load both ways.  Off the GPU / without the HIP library / for other dtypes
    it IS GraphConv."""

    def conv(self, block, h):
        if _fused_layers_apply(block, h) or _half_rows_apply(block, h):
            return _FusedGraphConvFn.apply(h, self.fc.weight, self.fc.bias, block, block.number_of_dst_nodes())
        return super().conv(block, h)


class _WeightedMeanCatFn(th.autograd.Function):
    """z = [sum_e w_e q_u / max(sum_e w_e, 1) | h_dst]: PinSAGE's weighted neighbour mean written straight into the left
    column block of the concatenation (weight sums by fgnn_block_degrees, the division inside
    fgnn_block_aggregate_scaled), the destinations' own rows copied into the right block.  Backward: the left block of
    the upstream gradient is read in place through its row stride.  The edge weights are visit counts: no gradient."""

    @staticmethod
    def forward(ctx, q, h, block, w, num_dst):
        from fgnn_hip.nn import aggregate_scaled_into, block_degrees
        hidden, din = q.shape[1], h.shape[1]
        _, ws = block_degrees(block.row, block.col, q.shape[0], num_dst, edge_weight=w, want_src=False)
        z = th.empty((num_dst, hidden + din), dtype=q.dtype, device=q.device)
        z[:, :hidden] = 0
        aggregate_scaled_into(z[:, :hidden], q if q.stride(1) == 1 else q.contiguous(), block.row, block.col, w,
                              dst_deg=ws, dst_mode=2)
        z[:, hidden:] = h[:num_dst]  # (fp16 input features: only these num_dst rows are upcast)
        ctx.save_for_backward(block.row, block.col, w, ws)
        ctx.shape = (q.shape[0], h.shape[0], hidden, din)
        return z

    @staticmethod
    def backward(ctx, gz):
        from fgnn_hip.nn import aggregate_scaled_into
        row, col, w, ws = ctx.saved_tensors
        nq, nh, hidden, din = ctx.shape
        if gz.stride(1) != 1 or gz.stride(0) < gz.shape[1]:
            gz = gz.contiguous()
        gq = gh = None
        if ctx.needs_input_grad[0]:
            gq = th.zeros((nq, hidden), dtype=gz.dtype, device=gz.device)
            aggregate_scaled_into(gq, gz[:, :hidden], col, row, w, src_deg=ws, src_mode=2)
        if ctx.needs_input_grad[1]:
            gh = th.zeros((nh, din), dtype=gz.dtype, device=gz.device)
            gh[:gz.shape[0]] = gz[:, hidden:]
        return gq, gh, None, None, None


class FusedWeightedSAGEConv(WeightedSAGEConv):
    """WeightedSAGEConv on the fused kernels: the weighted mean lands in its half of the concatenation in one launch
    (_WeightedMeanCatFn), ReLU + row normalisation are one launch each way (fgnn_relu_l2norm); the GEMMs and the two
    dropouts stay torch ops.  Same parameters under the same names (Q.*, W.*); off the GPU / without the HIP library /
    for other dtypes it IS WeightedSAGEConv.  fp16 input features: what this layer aggregates is q = relu(Q h), so
    the Q GEMM still needs fp32 operands (half-precision GEMMs are not built) and upcasts h for itself; the
    destinations' own rows go from the fp16 tensor straight into the concatenation."""

    def forward(self, block, h):
        if not (_fused_layers_apply(block, h) or _half_rows_apply(block, h)):
            return super().forward(block, h)
        from fgnn_hip.nn import relu_l2norm
        w = block.edata["weights"].to(th.float32)
        q = F.relu(self.Q(self.dropout(h.float())))  # (.float() of an fp32 tensor is the tensor itself)
        z = _WeightedMeanCatFn.apply(q, h, block, w.contiguous(), block.number_of_dst_nodes())
        return relu_l2norm(self.W(self.dropout(z)))


class GATConv(nn.Module):
    """dgl.nn.GATConv on a block as the reference's GAT uses it (example/samgraph/train_gat.py), op by op: one `fc` for
    sources and destinations (feat_dst = feat_src[:num_dst]), additive attention el[u] + er[v] through LeakyReLU,
    softmax over every destination's incoming edges per head, attention dropout, weighted sum, residual, bias,
    activation.  A destination without an edge gets residual + bias only (allow_zero_in_degree=True).  Parameter names
    and shapes are DGL's (fc.weight, attn_l / attn_r [1, H, F], bias [H F], res_fc.weight when the residual needs a
    projection), so the reference's checkpoints load.  Returns [num_dst, H, F]."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False,
                 activation=None):
        super().__init__()
        self.in_feats, self.out_feats, self.num_heads = in_feats, out_feats, num_heads
        self.fc = TallLinear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(th.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(th.empty(1, num_heads, out_feats))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.negative_slope = negative_slope
        self.res_fc = None
        if residual:
            self.res_fc = (TallLinear(in_feats, out_feats * num_heads, bias=False) if in_feats != out_feats * num_heads
                           else nn.Identity())
        self.bias = nn.Parameter(th.zeros(num_heads * out_feats))
        self.activation = activation
        gain = nn.init.calculate_gain("relu")  # DGL's reset_parameters
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)

    def project(self, block, h):
        """(h_dst after feature dropout, feat_src [num_src, H, F], el [num_src, H], er [num_dst, H])"""
        num_dst = block.number_of_dst_nodes()
        h = self.feat_drop(h)
        feat = self.fc(h).view(-1, self.num_heads, self.out_feats)
        el = (feat * self.attn_l).sum(-1)
        er = (feat[:num_dst] * self.attn_r).sum(-1)
        return h[:num_dst], feat, el, er

    def finish(self, rst, h_dst, biased=False):
        """residual, bias (unless it is in rst already) and activation"""
        if self.res_fc is not None and not biased:
            rst = rst + self.res_fc(h_dst).view(h_dst.shape[0], -1, self.out_feats)
        if not biased:
            rst = rst + self.bias.view(1, self.num_heads, self.out_feats)
        return self.activation(rst) if self.activation else rst

    def forward(self, block, h):
        num_dst = block.number_of_dst_nodes()
        h_dst, feat, el, er = self.project(block, h)
        row, col = block.row.long(), block.col.long()
        e = F.leaky_relu(el[row] + er[col], self.negative_slope)  # [E, H]
        # edge softmax: per (destination, head) max, exp, sum -- destinations without an edge are never indexed
        m = th.full((num_dst, self.num_heads), float("-inf"), dtype=e.dtype, device=e.device)
        # (the max only guards exp against overflow, the softmax does not depend on it: no gradient through it)
        m = m.scatter_reduce(0, col.unsqueeze(1).expand_as(e), e.detach(), reduce="amax", include_self=True)
        p = th.exp(e - m[col])
        z = th.zeros((num_dst, self.num_heads), dtype=e.dtype, device=e.device).index_add_(0, col, p)
        a = self.attn_drop(p / z[col])
        rst = th.zeros((num_dst, self.num_heads, self.out_feats), dtype=feat.dtype, device=feat.device)
        rst = rst.index_add_(0, col, feat[row] * a.unsqueeze(-1))
        return self.finish(rst, h_dst)


class FusedGATConv(GATConv):
    """GATConv with everything between the projections and the activation -- scores, edge softmax, attention dropout,
    aggregation -- as one autograd node on the kernels of csrc/gat_attention.hip (fgnn_hip.nn.gat_attention): no E x H x
    F tensor is written in either direction.  The bias (and the residual) is pre-filled into the node's output, which
    the kernel accumulates into.  Same parameters under the same names; off the GPU / without the HIP library / for
    other dtypes it IS GATConv.  `dropout_key` = (seed, d_step, tag) of the attention mask, set by the model before
    every forward."""

    dropout_key = (0x5A4D47, None, 0)

    def forward(self, block, h):
        if not _fused_layers_apply(block, h):
            return super().forward(block, h)
        from fgnn_hip.nn import gat_attention
        num_dst = block.number_of_dst_nodes()
        h_dst, feat, el, er = self.project(block, h)
        bias = self.bias.view(1, self.num_heads, self.out_feats)
        if self.res_fc is not None:
            out = self.res_fc(h_dst).view(num_dst, self.num_heads, self.out_feats) + bias
        else:
            out = bias.expand(num_dst, -1, -1).contiguous()
        seed, d_step, tag = self.dropout_key
        rst = gat_attention(feat, el, er, block.row, block.col, num_dst, self.negative_slope, self.attn_drop.p,
                            self.training, seed, d_step, tag, out=out)
        return self.finish(rst, h_dst, biased=True)


class GAT(nn.Module):
    """the reference's GAT (example/samgraph/train_gat.py): inner layers of `heads` heads with n_hidden // heads
    features each, flattened (layer width n_hidden: 256 = 8 x 32), ELU; the last layer `out_heads` heads of n_classes,
    averaged.  Feature dropout `dropout` and attention dropout `attn_drop` (default: the same) in every layer."""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, dropout, fused=True, heads=8, out_heads=1,
                 attn_drop=None, negative_slope=0.2, residual=False):
        super().__init__()
        assert n_hidden % heads == 0, "n_hidden must be a multiple of heads"
        attn_drop = dropout if attn_drop is None else attn_drop
        conv = FusedGATConv if fused else GATConv
        self.fused = fused
        layers = []
        for i in range(n_layers):
            last = i == n_layers - 1
            layers.append(conv(in_feats if i == 0 else n_hidden, n_classes if last else n_hidden // heads,
                               out_heads if last else heads, dropout, attn_drop, negative_slope,
                               residual and i > 0, None if last else F.elu))
        self.layers = nn.ModuleList(layers)
        # as SAGE / GCN: a training loop that uses fgnn_hip.nn.Adam sets dropout_step to its device-side step count, which
        # then keys the attention masks (a replayed graph draws a fresh mask per step).  Unset: every forward takes a fresh
        # seed from a host-side counter (no device synchronisation; a captured forward replays ITS mask)
        self.dropout_step = None
        self.dropout_seed = 0x5A4D47
        self._host_draws = 0

    def forward(self, blocks, x):
        seed = self.dropout_seed
        if self.fused and self.dropout_step is None and self.training:
            self._host_draws += 1
            seed = (seed + 0x9E3779B97F4A7C15 * self._host_draws) & 0xFFFFFFFFFFFFFFFF
        h = input_rows(self.layers[0], blocks[0], x)  # fp16 features: GAT upcasts once with torch
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            if self.fused:
                layer.dropout_key = (seed, self.dropout_step, i)
            h = layer(block, h)
            h = h.mean(1) if i == len(self.layers) - 1 else h.flatten(1)
        return h


class SAGE(nn.Module):
    def __init__(self, in_feats, n_hidden, n_classes, n_layers, dropout, fused=True):
        super().__init__()
        dims = [in_feats] + [n_hidden] * (n_layers - 1) + [n_classes]
        # fused=False: the op-by-op layer (two nn.Linear-like maps per layer, the layout a DGL SAGEConv checkpoint has)
        conv = FusedSAGEConv if fused else SAGEConvMean
        self.layers = nn.ModuleList(conv(dims[i], dims[i + 1]) for i in range(n_layers))
        self.dropout = nn.Dropout(dropout)
        # set by a training loop that uses fgnn_hip.nn.Adam: its device-side step count keys the dropout masks, so
        # ReLU + dropout run as ONE launch (fgnn_relu_dropout) and a replayed graph still draws a fresh mask per step
        self.dropout_step = None
        self.dropout_seed = 0x5A4D47

    def forward(self, blocks, x):
        h = input_rows(self.layers[0], blocks[0], x)
        for l, (layer, block) in enumerate(zip(self.layers, blocks)):
            h = layer(block, h)
            if l != len(self.layers) - 1:
                if self.dropout_step is not None and h.is_cuda and h.dtype == th.float32 and h.numel() % 4 == 0:
                    from fgnn_hip.nn import relu_dropout
                    h = relu_dropout(h, self.dropout.p, self.training, self.dropout_seed, self.dropout_step, l)
                else:
                    h = self.dropout(F.relu(h))
        return h


class GCN(nn.Module):
    def __init__(self, in_feats, n_hidden, n_classes, n_layers, dropout, fused=True):
        super().__init__()
        dims = [in_feats] + [n_hidden] * (n_layers - 1) + [n_classes]
        # fused=False: the op-by-op layer (a dozen torch ops around one aggregation launch)
        conv = FusedGraphConv if fused else GraphConv
        self.fused = fused
        self.layers = nn.ModuleList(conv(dims[i], dims[i + 1], F.relu if i < n_layers - 1 else None)
                                    for i in range(n_layers))
        self.dropout = nn.Dropout(dropout)
        # as SAGE: set by a training loop that uses fgnn_hip.nn.Adam; the fused model then runs an inner layer's ReLU and
        # the next layer's dropout as ONE launch (fgnn_relu_dropout) with a mask keyed by the device-side step count
        self.dropout_step = None
        self.dropout_seed = 0x5A4D47

    def forward(self, blocks, x):
        h = input_rows(self.layers[0], blocks[0], x)
        if self.fused and self.dropout_step is not None:
            from fgnn_hip.nn import relu_dropout
            for i, (layer, block) in enumerate(zip(self.layers, blocks)):
                if i == len(self.layers) - 1:
                    h = layer(block, h)
                    break
                h = layer(block, h, activate=False)
                if h.is_cuda and h.dtype == th.float32 and h.numel() % 4 == 0:
                    h = relu_dropout(h, self.dropout.p, self.training, self.dropout_seed, self.dropout_step, i)
                else:
                    h = self.dropout(F.relu(h))
            return h
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            if i != 0:
                h = self.dropout(h)
            h = layer(block, h)
        return h


class PinSAGE(nn.Module):
    def __init__(self, in_feats, n_hidden, n_classes, n_layers, dropout, fused=True):
        super().__init__()
        dims = [in_feats] + [n_hidden] * (n_layers - 1) + [n_classes]
        conv = FusedWeightedSAGEConv if fused else WeightedSAGEConv
        self.layers = nn.ModuleList(conv(dims[i], n_hidden, dims[i + 1], dropout) for i in range(n_layers))

    def forward(self, blocks, x):
        h = input_rows(self.layers[0], blocks[0], x)
        for layer, block in zip(self.layers, blocks):
            h = layer(block, h)
        return h


MODELS = {"graphsage": SAGE, "gcn": GCN, "pinsage": PinSAGE, "gat": GAT}
