"""Exact layer-wise inference on the full graph: layer 1 for all N nodes over the whole CSR, then layer 2 from that --
no sampling, no neighbourhood explosion, the model's prediction (or embedding) for every node.  The counterpart of
`model.inference` in the reference's DGL baselines.

On the GPU the aggregation is fgnn_csr_aggregate (csrc/csr_aggregate.hip; fgnn_hip.nn.csr_aggregate_into): one wave per
CSR row, sums in registers, one store -- no destination array per edge, no zero fill, no float atomics, and a node's
result is bit for bit the same whatever chunk it is computed in.  Per chunk of `batch_rows` destination rows:
    SAGE   z = [h[a:b] | mean of the neighbours' rows]   the mean written straight into z[:, din:] (dst_mode 2 with the
           row length as the degree), then ONE addmm with [W_self | W_neigh]
    GCN    agg = in_deg^-1/2 * sum out_deg^-1/2 h[u]      out_deg = a node's occurrences in `indices`, computed once per
           call; in_deg = the row length; then one addmm; ReLU between layers
On CPU tensors, or without the kernel library, the same function runs op by op in torch: what the CPU tests exercise
and what the fused path is compared with.  Intermediate activations are fp32 [N, hidden] on the device; fp16 features
are read as they are by the first layer (no fp32 copy of the feature matrix is made).

GAT has a pass of its own, gat_layerwise_inference: an edge-softmax over CSR rows is not a weighted sum.  Per layer it
projects all N rows in chunks (feat = fc(h) as [N, H, F], el, er), then per chunk of destination rows runs
fgnn_csr_gat_attention (csrc/csr_gat_attention.hip; fgnn_hip.nn.csr_gat_attention_into: one wave per CSR row, max, sum
and weighted sums in registers, no E x H scratch, no float atomics, bit-reproducible rows) and the layer's own finish
(residual, bias, ELU).  full_graph_inference picks the pass by the model's class; it is what the training scripts call.

Not built: PinSAGE (its neighbourhood is defined by random walks, not by the CSR) raises NotImplementedError;
intermediate activations in fp16; inference partitioned over several GPUs."""
import numpy as np
import torch as th
import torch.nn.functional as F

import models  # (classes are looked up per call: a reloaded `models` module must still be recognised)

try:
    from fgnn_hip import nn as _nn
    from fgnn_hip.lib import FgnnError as _FgnnError
except ImportError:
    _nn = None


def _library():
    """fgnn_hip.nn if the kernel library can be loaded, else None"""
    if _nn is None:
        return None
    try:
        _nn._lib.load()
    except (_FgnnError, OSError):
        return None
    return _nn


def _as_ids(a, device):
    """a CSR array as an int32-viewed u32 tensor on `device`"""
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a)
        a = th.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.astype(np.int32))
    if a.dtype != th.int32:
        a = a.to(th.int32)
    return a.to(device).contiguous()


def _u32(t):
    """the values of an int32-viewed u32 tensor as int64"""
    return t.long() & 0xFFFFFFFF


def _on_device(model, indptr, indices, feat, device):
    """(device, the model's dtype, indptr, indices, feat, N) with graph and features moved to `device` (default: the
    model's)"""
    param = next(model.parameters())
    device = th.device(device) if device is not None else param.device
    dtype = param.dtype
    if isinstance(feat, np.ndarray):
        feat = th.from_numpy(feat)
    assert feat.dtype in (th.float32, th.float16) or feat.dtype == dtype
    indptr, indices, h = _as_ids(indptr, device), _as_ids(indices, device), feat.to(device)
    n = indptr.numel() - 1
    assert h.shape[0] == n
    return device, dtype, indptr, indices, h, n


def _longest_chunk(indptr64, n, batch_rows, device):
    """edges of the longest chunk of batch_rows rows: one workspace size for all chunks (one device-to-host copy of the
    chunk boundaries per call, outside the per-chunk path)"""
    cuts = indptr64[th.arange(0, n + batch_rows, batch_rows, device=device).clamp(max=n)]
    return int((cuts[1:] - cuts[:-1]).max()) if n else 0


def _layer_params(model, layer):
    """(W [out, k in], bias) of a layer in the fused layout: SAGE [W_self | W_neigh], GCN fc"""
    if isinstance(model, models.GCN):
        return layer.fc.weight, layer.fc.bias
    if isinstance(layer, models.FusedSAGEConv):
        return layer.weight, layer.bias
    return th.cat([layer.fc_self.weight, layer.fc_neigh.weight], 1), layer.fc_neigh.bias


def _chunk_op_by_op(sage, h, indptr64, indices64, a, b, src_factor, dtype):
    """z of the destination rows [a, b) with torch ops: the neighbour sums by index_add_, the degree factors applied as
    the op-by-op layers of models.py apply them"""
    p0, p1 = int(indptr64[a]), int(indptr64[b])
    src = indices64[p0:p1]
    k = indptr64[a + 1:b + 1] - indptr64[a:b]
    dst = th.repeat_interleave(th.arange(b - a, device=h.device), k)
    msg = h[src].to(dtype)
    if not sage:
        msg = msg * src_factor[src].unsqueeze(1)
    agg = th.zeros((b - a, h.shape[1]), dtype=dtype, device=h.device).index_add_(0, dst, msg)
    deg = k.to(dtype).clamp(min=1)
    if sage:
        return th.cat([h[a:b].to(dtype), agg / deg.unsqueeze(1)], 1)
    return agg * deg.pow(-0.5).unsqueeze(1)


def layerwise_inference(model, indptr, indices, feat, batch_rows=65536, device=None):
    """[N, n_classes] fp32 logits of `model` (models.SAGE or models.GCN, fused or op-by-op layers) for every node of the
    graph (indptr, indices: the CSR, int32-viewed u32 tensors or u32 arrays; row v lists the nodes v aggregates from),
    feat [N, D] fp32 or fp16.  (A float64 model computes and answers in float64, on the op-by-op path.)  device: where to compute (default: the model's); graph and features are moved there if
    they are elsewhere.  The model runs in eval() mode under no_grad -- no dropout -- and gets its training flag
    back."""
    if isinstance(model, models.PinSAGE):
        raise NotImplementedError("layer-wise inference of PinSAGE: its neighbourhood is defined by random walks, not by "
                                  "the CSR rows this pass aggregates over")
    if isinstance(model, models.GAT):
        raise NotImplementedError("layer-wise inference of GAT is an edge-softmax over CSR rows, not this pass's weighted "
                                  "sum: call gat_layerwise_inference (or full_graph_inference)")
    if not isinstance(model, (models.SAGE, models.GCN)):
        raise NotImplementedError("layer-wise inference knows models.SAGE and models.GCN, not %s" % type(model).__name__)
    sage = isinstance(model, models.SAGE)
    device, dtype, indptr, indices, h, n = _on_device(model, indptr, indices, feat, device)
    assert batch_rows >= 1
    nn = _library() if device.type == "cuda" and dtype == th.float32 else None
    was_training = model.training
    model.eval()
    try:
        with th.no_grad():
            indptr64 = _u32(indptr)
            src_factor = src_deg = None
            if not sage:  # GCN: out-degree = occurrences in indices, once per graph (not the hot path)
                src_deg = th.bincount(_u32(indices), minlength=n).to(th.float32 if nn else dtype)
                src_factor = src_deg.clamp(min=1).pow(-0.5)
            if nn is None:
                indices64 = _u32(indices)
            else:
                max_edges = _longest_chunk(indptr64, n, batch_rows, device)
                if h.stride(1) != 1:
                    h = h.contiguous()
            for li, layer in enumerate(model.layers):
                W, bias = _layer_params(model, layer)
                din = h.shape[1]
                out = th.empty((n, W.shape[0]), dtype=th.float32 if nn else dtype, device=device)
                for a in range(0, n, batch_rows):
                    b = min(a + batch_rows, n)
                    if nn is None:
                        z = _chunk_op_by_op(sage, h, indptr64, indices64, a, b, src_factor, dtype)
                    elif sage:
                        z = th.empty((b - a, 2 * din), dtype=th.float32, device=device)
                        z[:, :din] = h[a:b]  # (fp16 features: only these rows are upcast)
                        nn.csr_aggregate_into(z[:, din:], h, indptr, indices, first=a, count=b - a, dst_mode=2,
                                              max_edges=max_edges)
                    else:
                        z = th.empty((b - a, din), dtype=th.float32, device=device)
                        nn.csr_aggregate_into(z, h, indptr, indices, first=a, count=b - a, src_deg=src_deg, src_mode=1,
                                              dst_mode=1, max_edges=max_edges)
                    th.addmm(bias, z, W.t(), out=out[a:b])
                h = out if li == len(model.layers) - 1 else th.relu_(out)
    finally:
        model.train(was_training)
    return h


def _gat_chunk_op_by_op(feat, el, er, indptr64, indices64, a, b, slope):
    """the attention sums [b - a, H, F] of the destination rows [a, b) with torch ops, as models.GATConv.forward computes
    them on a block: scores, per-(destination, head) max, exp, sum, weighted sum; rows without a neighbour stay zero"""
    p0, p1 = int(indptr64[a]), int(indptr64[b])
    src = indices64[p0:p1]
    k = indptr64[a + 1:b + 1] - indptr64[a:b]
    dst = th.repeat_interleave(th.arange(b - a, device=feat.device), k)
    e = F.leaky_relu(el[src] + er[a:b][dst], slope)
    m = th.full((b - a, e.shape[1]), float("-inf"), dtype=e.dtype, device=e.device)
    m = m.scatter_reduce(0, dst.unsqueeze(1).expand_as(e), e, reduce="amax", include_self=True)
    p = th.exp(e - m[dst])
    z = th.zeros_like(m).index_add_(0, dst, p)
    alpha = p / z[dst]
    rst = th.zeros((b - a,) + tuple(feat.shape[1:]), dtype=feat.dtype, device=feat.device)
    return rst.index_add_(0, dst, feat[src] * alpha.unsqueeze(-1))


def gat_layerwise_inference(model, indptr, indices, feat, batch_rows=65536, device=None):
    """[N, n_classes] logits of `model` (models.GAT, fused or op-by-op layers, with or without residual) for every node
    of the graph; arguments and conventions as layerwise_inference (fp16 features are upcast per chunk by torch, as
    GAT.forward upcasts them; a float64 model computes and answers in float64).  Per layer: feat = fc(h) [N, H, F], el
    and er for all N rows in chunks of batch_rows; then per chunk of destination rows the attention sums over their whole
    CSR rows -- on the GPU with an fp32 model fgnn_hip.nn.csr_gat_attention_into, else (CPU tensors, no kernel
    library, float64, more heads than the kernel stages) torch ops -- and the layer's finish: residual from h[a:b],
    bias, ELU; flatten(1) between layers, mean(1) over the heads of the last."""
    if not isinstance(model, models.GAT):
        raise NotImplementedError("gat_layerwise_inference knows models.GAT, not %s" % type(model).__name__)
    device, dtype, indptr, indices, h, n = _on_device(model, indptr, indices, feat, device)
    assert batch_rows >= 1
    nn = _library() if device.type == "cuda" and dtype == th.float32 else None
    was_training = model.training
    model.eval()
    try:
        with th.no_grad():
            indptr64 = _u32(indptr)
            indices64 = _u32(indices)
            max_edges = _longest_chunk(indptr64, n, batch_rows, device) if nn else 0
            chunks = [(a, min(a + batch_rows, n)) for a in range(0, n, batch_rows)]
            for li, layer in enumerate(model.layers):
                H, Fo = layer.num_heads, layer.out_feats
                kernel = nn is not None and H <= nn.csr_gat_max_heads()
                proj = th.empty((n, H, Fo), dtype=dtype, device=device)
                el, er = (th.empty((n, H), dtype=dtype, device=device) for _ in range(2))
                for a, b in chunks:
                    f = layer.fc(h[a:b].to(dtype)).view(b - a, H, Fo)
                    proj[a:b] = f
                    th.sum(f * layer.attn_l, -1, out=el[a:b])
                    th.sum(f * layer.attn_r, -1, out=er[a:b])
                last = li == len(model.layers) - 1
                out = th.empty((n, Fo if last else H * Fo), dtype=dtype, device=device)
                for a, b in chunks:
                    if kernel:
                        rst = th.empty((b - a, H, Fo), dtype=th.float32, device=device)
                        nn.csr_gat_attention_into(rst, proj, el, er, indptr, indices, first=a, count=b - a,
                                                  negative_slope=layer.negative_slope, max_edges=max_edges)
                    else:
                        rst = _gat_chunk_op_by_op(proj, el, er, indptr64, indices64, a, b, layer.negative_slope)
                    rst = layer.finish(rst, h[a:b].to(dtype))
                    out[a:b] = rst.mean(1) if last else rst.flatten(1)
                h = out
    finally:
        model.train(was_training)
    return h


def full_graph_inference(model, indptr, indices, feat, batch_rows=65536, device=None):
    """the exact prediction of `model` for every node by the pass its class has: gat_layerwise_inference for models.GAT,
    layerwise_inference for everything else (which refuses what it cannot do, models.PinSAGE, with a reason)"""
    fn = gat_layerwise_inference if isinstance(model, models.GAT) else layerwise_inference
    return fn(model, indptr, indices, feat, batch_rows=batch_rows, device=device)
