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

Not built: PinSAGE (its neighbourhood is defined by random walks, not by the CSR) and GAT (it needs an edge-softmax over
CSR rows, a kernel of its own) raise NotImplementedError; intermediate activations in fp16; inference partitioned over
several GPUs."""
import numpy as np
import torch as th

from models import GAT, GCN, SAGE, FusedSAGEConv, PinSAGE

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


def _layer_params(model, layer):
    """(W [out, k in], bias) of a layer in the fused layout: SAGE [W_self | W_neigh], GCN fc"""
    if isinstance(model, GCN):
        return layer.fc.weight, layer.fc.bias
    if isinstance(layer, FusedSAGEConv):
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
    if isinstance(model, PinSAGE):
        raise NotImplementedError("layer-wise inference of PinSAGE: its neighbourhood is defined by random walks, not by "
                                  "the CSR rows this pass aggregates over")
    if isinstance(model, GAT):
        raise NotImplementedError("layer-wise inference of GAT needs an edge-softmax over CSR rows, a kernel of its own "
                                  "that is not built")
    if not isinstance(model, (SAGE, GCN)):
        raise NotImplementedError("layer-wise inference knows models.SAGE and models.GCN, not %s" % type(model).__name__)
    sage = isinstance(model, SAGE)
    param = next(model.parameters())
    device = th.device(device) if device is not None else param.device
    dtype = param.dtype
    if isinstance(feat, np.ndarray):
        feat = th.from_numpy(feat)
    assert feat.dtype in (th.float32, th.float16) or feat.dtype == dtype
    indptr, indices, h = _as_ids(indptr, device), _as_ids(indices, device), feat.to(device)
    n = indptr.numel() - 1
    assert h.shape[0] == n and batch_rows >= 1
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
                # one workspace size for all chunks: the longest chunk's edges (one device-to-host copy of the chunk
                # boundaries per call, outside the per-chunk path)
                cuts = indptr64[th.arange(0, n + batch_rows, batch_rows, device=device).clamp(max=n)]
                max_edges = int((cuts[1:] - cuts[:-1]).max()) if n else 0
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
