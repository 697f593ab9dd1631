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
A pool SAGE (models.SAGE(aggregator="pool")) is not a mean model although its layers have fc_self / fc_neigh too: per
layer p = relu(fc_pool(h)) for all nodes in chunks, the row maxima over the CSR rows by a torch scatter amax (on the CPU
and on the GPU alike), then the layer's GEMM on z = [h[a:b] | max].  A CSR max kernel with the hub queue of csr_queue.h
is the natural follow-up and is not built.
On CPU tensors, or without the kernel library, the same function runs op by op in torch: what the CPU tests exercise
and what the fused path is compared with.  Intermediate activations are fp32 [N, hidden] on the device; fp16 features
are read as they are by the first layer (no fp32 copy of the feature matrix is made).

GAT has a pass of its own, gat_layerwise_inference: an edge-softmax over CSR rows is not a weighted sum.  Per layer it
projects all N rows in chunks (feat = fc(h) as [N, H, F], el, er), then per chunk of destination rows runs
fgnn_csr_gat_attention (csrc/csr_gat_attention.hip; fgnn_hip.nn.csr_gat_attention_into: one wave per CSR row, max, sum
and weighted sums in registers, no E x H scratch, no float atomics, bit-reproducible rows) and the layer's own finish
(residual, bias, ELU).

GATv2 has gatv2_layerwise_inference, the same pass on its own kernel: the score attn . leaky_relu(fs[u] + fd[v]) is a
reduction over the neighbour's whole projected row, so fgnn_csr_gatv2_attention (csrc/csr_gatv2_attention.hip;
fgnn_hip.nn.csr_gatv2_attention_into) walks a CSR row ONCE with an online softmax in fixed blocks -- every fs row is read
once, same guarantees.  full_graph_inference picks the pass by the model's class; it is what the training scripts call.

Not built: PinSAGE (its neighbourhood is defined by random walks, not by the CSR) raises NotImplementedError;
intermediate activations in fp16; inference partitioned over several GPUs."""
import types

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


def _on_device(model, indptr, indices, feat, device, q8_ok=False):
    """(device, the model's dtype, indptr, indices, feat, N) with graph and features moved to `device` (default: the
    model's).  q8_ok: the caller also reads a q8 feature table (uint8 [N, S], csrc/q8_rows.h)"""
    param = next(model.parameters())
    device = th.device(device) if device is not None else param.device
    dtype = param.dtype
    if isinstance(feat, np.ndarray):
        feat = th.from_numpy(feat)
    assert feat.dtype in (th.float32, th.float16) or feat.dtype == dtype or (q8_ok and feat.dtype == th.uint8)
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
    if isinstance(layer, (models.FusedSAGEConv, models.FusedSAGEPoolConv)):
        return layer.weight, layer.bias
    return th.cat([layer.fc_self.weight, layer.fc_neigh.weight], 1), layer.fc_neigh.bias


def _pool_rows(layer, h, indptr64, indices64, n, batch_rows, dtype):
    """the max-pooling half of a pool SAGE layer for all n nodes, [n, din]: p = relu(fc_pool(h)) in chunks of batch_rows
    (fp16 / q8 rows upcast or decoded per chunk: fc_pool is a GEMM), then per chunk of destination rows the maxima over
    their CSR rows by one torch scatter amax into zeros (a row without a neighbour keeps 0) -- on the CPU and on the GPU
    alike.  That scatter materialises the chunk's p[src] rows: a CSR max kernel with the hub queue of csr_queue.h is the
    natural follow-up and is not built."""
    din = layer.fc_pool.in_features
    p = th.empty((n, din), dtype=dtype, device=h.device)
    for a in range(0, n, batch_rows):
        b = min(a + batch_rows, n)
        x = models.decode_q8(h[a:b], din) if h.dtype == th.uint8 else h[a:b].to(dtype)
        p[a:b] = th.relu_(layer.fc_pool(x))
    m = th.zeros((n, din), dtype=dtype, device=h.device)
    for a in range(0, n, batch_rows):
        b = min(a + batch_rows, n)
        src, dst = _chunk_edges(indptr64, indices64, a, b)
        m[a:b].scatter_reduce_(0, dst.unsqueeze(1).expand(-1, din), p[src], "amax", include_self=True)
    return m


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
    feat [N, D] fp32 or fp16, or a q8 table (uint8 [N, S]: the first layer's CSR aggregation reads the codes as they are,
    fgnn_csr_aggregate_q8; GPU only).  (A float64 model computes and answers in float64, on the op-by-op path.)  device: where to compute (default: the model's); graph and features are moved there if
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
    pool = sage and getattr(model, "aggregator", "mean") == "pool"  # a pool layer has fc_self / fc_neigh too: not a mean
    device, dtype, indptr, indices, h, n = _on_device(model, indptr, indices, feat, device, q8_ok=True)
    assert batch_rows >= 1
    nn = _library() if device.type == "cuda" and dtype == th.float32 else None
    if h.dtype == th.uint8 and nn is None:
        raise NotImplementedError("a q8 feature table is read by the HIP kernels only: fp32 model on a GPU")
    was_training = model.training
    model.eval()
    try:
        with th.no_grad():
            indptr64 = _u32(indptr)
            src_factor = src_deg = None
            if not sage:  # GCN: out-degree = occurrences in indices, once per graph (not the hot path)
                src_deg = th.bincount(_u32(indices), minlength=n).to(th.float32 if nn else dtype)
                src_factor = src_deg.clamp(min=1).pow(-0.5)
            if nn is None or pool:
                indices64 = _u32(indices)
            if nn is not None:
                max_edges = _longest_chunk(indptr64, n, batch_rows, device)
                if h.stride(1) != 1:
                    h = h.contiguous()
            for li, layer in enumerate(model.layers):
                W, bias = _layer_params(model, layer)
                din = W.shape[1] // 2 if sage else W.shape[1]  # (not h.shape[1]: q8 rows are S bytes wide)
                out = th.empty((n, W.shape[0]), dtype=th.float32 if nn else dtype, device=device)
                pooled = _pool_rows(layer, h, indptr64, indices64, n, batch_rows, dtype) if pool else None
                for a in range(0, n, batch_rows):
                    b = min(a + batch_rows, n)
                    if pool:
                        own = models.decode_q8(h[a:b], din) if h.dtype == th.uint8 else h[a:b].to(dtype)
                        z = th.cat([own, pooled[a:b]], 1)
                    elif nn is None:
                        z = _chunk_op_by_op(sage, h, indptr64, indices64, a, b, src_factor, dtype)
                    elif sage:
                        z = th.empty((b - a, 2 * din), dtype=th.float32, device=device)
                        if h.dtype == th.uint8:  # q8 features: only these rows are decoded
                            models.decode_q8(h[a:b], din, out=z[:, :din])
                        else:
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


def _chunk_edges(indptr64, indices64, a, b):
    """(src, dst) of the edges of the destination rows [a, b): the neighbour ids and the row's position in the chunk"""
    p0, p1 = int(indptr64[a]), int(indptr64[b])
    k = indptr64[a + 1:b + 1] - indptr64[a:b]
    return indices64[p0:p1], th.repeat_interleave(th.arange(b - a, device=indptr64.device), k)


def _edge_softmax_sum(e, msg, dst, rows):
    """[rows, H, F]: the sums of msg [E, H, F] weighted by the softmax of the scores e [E, H] over every destination's
    edges, as the op-by-op layers of models.py compute them on a block: per-(destination, head) max, exp, sum, weighted
    sum; rows without a neighbour stay zero"""
    m = th.full((rows, e.shape[1]), float("-inf"), dtype=e.dtype, device=e.device)
    m = m.scatter_reduce(0, dst.unsqueeze(1).expand_as(e), e, reduce="amax", include_self=True)
    p = th.exp(e - m[dst])
    z = th.zeros_like(m).index_add_(0, dst, p)
    alpha = p / z[dst]
    rst = th.zeros((rows,) + tuple(msg.shape[1:]), dtype=msg.dtype, device=msg.device)
    return rst.index_add_(0, dst, msg * alpha.unsqueeze(-1))


def _gat_chunk_op_by_op(feat, el, er, indptr64, indices64, a, b, slope):
    """the attention sums [b - a, H, F] of the destination rows [a, b) with torch ops, as models.GATConv.forward computes
    them on a block"""
    src, dst = _chunk_edges(indptr64, indices64, a, b)
    return _edge_softmax_sum(F.leaky_relu(el[src] + er[a:b][dst], slope), feat[src], dst, b - a)


def _gatv2_chunk_op_by_op(fs, fd, attn, indptr64, indices64, a, b, slope):
    """the same for models.GATv2Conv.forward: the score is attn . leaky_relu(fs[u] + fd[v]), an E x H x F tensor per
    chunk"""
    src, dst = _chunk_edges(indptr64, indices64, a, b)
    fsr = fs[src]
    return _edge_softmax_sum((F.leaky_relu(fsr + fd[a:b][dst], slope) * attn).sum(-1), fsr, dst, b - a)


def _attention_inference(model, indptr, indices, feat, batch_rows, device, project):
    """What the GAT and the GATv2 pass share.  Per layer `project(g, layer, h)` projects all N rows of h in g.chunks and
    returns attend(a, b), the attention sums [b - a, H, F] of the destination rows [a, b); then per chunk the layer's
    finish (residual from h[a:b], and what else the layer adds), flatten(1) between layers, mean(1) over the heads of
    the last.  g: the graph on the device (indptr, indices; indptr64, indices64 for torch indexing), n, chunks, dtype,
    device, max_edges of a chunk, and nn = fgnn_hip.nn where the kernels apply (GPU tensors, fp32 model, library
    loadable), else None."""
    g = types.SimpleNamespace()
    g.device, g.dtype, g.indptr, g.indices, h, g.n = _on_device(model, indptr, indices, feat, device)
    assert batch_rows >= 1
    g.nn = _library() if g.device.type == "cuda" and g.dtype == th.float32 else None
    was_training = model.training
    model.eval()
    try:
        with th.no_grad():
            g.indptr64 = _u32(g.indptr)
            g.indices64 = _u32(g.indices)
            g.max_edges = _longest_chunk(g.indptr64, g.n, batch_rows, g.device) if g.nn else 0
            g.chunks = [(a, min(a + batch_rows, g.n)) for a in range(0, g.n, batch_rows)]
            for li, layer in enumerate(model.layers):
                H, Fo = layer.num_heads, layer.out_feats
                attend = project(g, layer, h)
                last = li == len(model.layers) - 1
                out = th.empty((g.n, Fo if last else H * Fo), dtype=g.dtype, device=g.device)
                for a, b in g.chunks:
                    rst = layer.finish(attend(a, b), h[a:b].to(g.dtype))
                    out[a:b] = rst.mean(1) if last else rst.flatten(1)
                h = out
    finally:
        model.train(was_training)
    return h


def _gat_project(g, layer, h):
    H, Fo = layer.num_heads, layer.out_feats
    kernel = g.nn is not None and H <= g.nn.csr_gat_max_heads()
    proj = th.empty((g.n, H, Fo), dtype=g.dtype, device=g.device)
    el, er = (th.empty((g.n, H), dtype=g.dtype, device=g.device) for _ in range(2))
    for a, b in g.chunks:
        f = layer.fc(h[a:b].to(g.dtype)).view(b - a, H, Fo)
        proj[a:b] = f
        th.sum(f * layer.attn_l, -1, out=el[a:b])
        th.sum(f * layer.attn_r, -1, out=er[a:b])

    def attend(a, b):
        if not kernel:
            return _gat_chunk_op_by_op(proj, el, er, g.indptr64, g.indices64, a, b, layer.negative_slope)
        rst = th.empty((b - a, H, Fo), dtype=th.float32, device=g.device)
        return g.nn.csr_gat_attention_into(rst, proj, el, er, g.indptr, g.indices, first=a, count=b - a,
                                           negative_slope=layer.negative_slope, max_edges=g.max_edges)
    return attend


def _gatv2_project(g, layer, h):
    H, Fo = layer.num_heads, layer.out_feats
    kernel = g.nn is not None and Fo <= g.nn.csr_gatv2_max_feats()
    fs = th.empty((g.n, H, Fo), dtype=g.dtype, device=g.device)
    fd = fs if layer.fc_dst is None else th.empty_like(fs)
    for a, b in g.chunks:
        x = h[a:b].to(g.dtype)
        fs[a:b] = layer.fc_src(x).view(b - a, H, Fo)
        if layer.fc_dst is not None:
            fd[a:b] = layer.fc_dst(x).view(b - a, H, Fo)
    attn = layer.attn.detach().contiguous()

    def attend(a, b):
        if not kernel:
            return _gatv2_chunk_op_by_op(fs, fd, attn, g.indptr64, g.indices64, a, b, layer.negative_slope)
        rst = th.empty((b - a, H, Fo), dtype=th.float32, device=g.device)
        return g.nn.csr_gatv2_attention_into(rst, fs, fd, attn, g.indptr, g.indices, first=a, count=b - a,
                                             negative_slope=layer.negative_slope, max_edges=g.max_edges)
    return attend


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
    return _attention_inference(model, indptr, indices, feat, batch_rows, device, _gat_project)


def gatv2_layerwise_inference(model, indptr, indices, feat, batch_rows=65536, device=None):
    """[N, n_classes] logits of `model` (models.GATv2, fused or op-by-op layers, with or without residual and
    share_weights) for every node of the graph; arguments and conventions as gat_layerwise_inference.  Per layer: fs =
    fc_src(h) [N, H, F] and fd = fc_dst(h) (fd is fs where the layer shares its weights) for all N rows in chunks of
    batch_rows; then per chunk of destination rows the attention sums over their whole CSR rows -- on the GPU with an
    fp32 model fgnn_hip.nn.csr_gatv2_attention_into (every fs row read once), else (CPU tensors, no kernel library,
    float64, more features per head than the kernel serves) torch ops -- and the layer's finish: residual from h[a:b],
    ELU; flatten(1) between layers, mean(1) over the heads of the last."""
    if not isinstance(model, models.GATv2):
        raise NotImplementedError("gatv2_layerwise_inference knows models.GATv2, not %s" % type(model).__name__)
    return _attention_inference(model, indptr, indices, feat, batch_rows, device, _gatv2_project)


def full_graph_inference(model, indptr, indices, feat, batch_rows=65536, device=None):
    """the exact prediction of `model` for every node by the pass its class has: gat_layerwise_inference for models.GAT,
    gatv2_layerwise_inference for models.GATv2, layerwise_inference for everything else (which refuses what it cannot
    do, models.PinSAGE, with a reason)"""
    fn = (gat_layerwise_inference if isinstance(model, models.GAT) else
          gatv2_layerwise_inference if isinstance(model, models.GATv2) else layerwise_inference)
    return fn(model, indptr, indices, feat, batch_rows=batch_rows, device=device)
