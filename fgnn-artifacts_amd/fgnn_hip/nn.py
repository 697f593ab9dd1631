"""torch.autograd wrapper of fgnn_block_aggregate (csrc/block_aggregate.hip): the message-passing step of the
DGL-free layers in examples/models.py.  out[col[e]] += w[e] * h[row[e]]; backward is the same kernel with the two
index arrays swapped.  Index tensors are the int32 row / col tensors the engine returns (no copies)."""
import ctypes as C

import torch

from . import lib as _lib


# Argument and return types of every entry point are declared once, in lib.SIGNATURES (applied by lib.load()): the calls
# below pass addresses (lib._ptr: None = null), plain numbers and the current stream of a tensor's device (lib._stream).
_ptr, _st = _lib._ptr, _lib._stream


def _aggregate(out, h, src_idx, dst_idx, weight, in_degree=None, scaling=None):
    """the one aggregation call: out[dst_idx[e]] += weight[e] * h[src_idx[e]] through fgnn_block_aggregate_ex (h
    contiguous; in_degree optional), or, with scaling = (src_deg, src_mode, dst_deg, dst_mode), through
    fgnn_block_aggregate_scaled (h with a row stride, degree factors inside).  h float16 (input features of a
    half-precision store): the _f16 twin of either, which upcasts the rows on load."""
    L = _lib.load()
    n, dim = src_idx.numel(), h.shape[1]
    f16 = "_f16" if h.dtype == torch.float16 else ""
    if scaling is None:
        what = "fgnn_block_aggregate_ex" + f16
        code = getattr(L, what)(_ptr(src_idx), _ptr(dst_idx), _ptr(weight), n, _ptr(h), dim, _ptr(out),
                                out.stride(0), _ptr(in_degree), _st(h))
    else:
        src_deg, src_mode, dst_deg, dst_mode = scaling
        what = "fgnn_block_aggregate_scaled" + f16
        code = getattr(L, what)(_ptr(src_idx), _ptr(dst_idx), _ptr(weight), n, _ptr(h), h.stride(0), dim, _ptr(out),
                                out.stride(0), _ptr(src_deg), src_mode, _ptr(dst_deg), dst_mode, _st(h))
    _lib._check(code, what)
    return out


class _BlockAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, row, col, w, num_dst):
        h = h.contiguous()
        out = torch.zeros((num_dst, h.shape[1]), dtype=torch.float32, device=h.device)
        _aggregate(out, h, row, col, w)
        ctx.save_for_backward(row, col, w if w is not None else torch.empty(0, device=h.device))
        ctx.has_w = w is not None
        ctx.num_src = h.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        row, col, w = ctx.saved_tensors
        grad_h = None
        if ctx.needs_input_grad[0]:
            g = grad_out.contiguous()
            grad_h = torch.zeros((ctx.num_src, g.shape[1]), dtype=torch.float32, device=g.device)
            _aggregate(grad_h, g, col, row, w if ctx.has_w else None)
        return grad_h, None, None, None, None


def block_aggregate(h, row, col, num_dst, edge_weight=None):
    """sum_e edge_weight[e] * h[row[e]] into out[col[e]] (fp32); h float32 [num_src, D] -- or float16 where it needs no
    gradient (input features of a half-precision store) --, row / col int32 [E]."""
    assert h.dtype == torch.float32 or (h.dtype == torch.float16 and not h.requires_grad)
    assert row.dtype == torch.int32 and col.dtype == torch.int32
    assert row.is_contiguous() and col.is_contiguous() and row.numel() == col.numel()
    if edge_weight is not None:
        edge_weight = edge_weight.to(torch.float32).contiguous()
    return _BlockAggregate.apply(h, row, col, edge_weight, num_dst)


def aggregate_into(out, h, src_idx, dst_idx, edge_weight=None, in_degree=None):
    """out[dst_idx[e]] += edge_weight[e] * h[src_idx[e]] into a caller-initialised fp32 tensor: no autograd, for layers
    that write their own backward (examples/models.py: FusedSAGEConv).  `out` may be a column block of a wider
    row-major matrix (unit stride inside a row); in_degree (fp32 [num_dst], caller-zeroed) receives the edge count of
    every destination on the way.  h: fp32, or fp16 rows that are upcast on load."""
    assert h.dtype in (torch.float32, torch.float16) and out.dtype == torch.float32 and h.is_contiguous()
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[1] == h.shape[1]
    assert src_idx.dtype == torch.int32 and dst_idx.dtype == torch.int32
    return _aggregate(out, h, src_idx, dst_idx, edge_weight, in_degree)


# ---- fused pieces of a GraphSAGE training step (csrc/train_ops.hip) ------------------------------------------------------
# One launch each for work a step otherwise spends two to four torch ops on: the step is replayed as a captured HIP
# graph (examples/graphed_step.py), where a node costs the GPU 15-20 us whatever it does.

def sage_finish_z(z, h, deg, num_dst, din):
    """z[:, :din] = h[:num_dst] (h fp32, or fp16 and upcast); inv = 1 / max(deg, 1); z[:, din:] *= inv.  Returns inv
    (fp32 [num_dst])."""
    assert h.dtype in (torch.float32, torch.float16)
    inv = torch.empty(num_dst, dtype=torch.float32, device=z.device)
    what = "fgnn_sage_finish_z" + ("_f16" if h.dtype == torch.float16 else "")
    _lib._check(getattr(_lib.load(), what)(_ptr(z), z.stride(0), _ptr(h), h.stride(0), _ptr(deg), _ptr(inv), num_dst, din,
                                           _st(z)), what)
    return inv


def sage_grad_prep(gz, inv, num_src, din):
    """(gh, gagg): gh[:num_dst] = gz[:, :din], gh[num_dst:] = 0; gagg = gz[:, din:] * inv[:, None]"""
    num_dst = gz.shape[0]
    gh = torch.empty((num_src, din), dtype=torch.float32, device=gz.device)
    gagg = torch.empty((num_dst, din), dtype=torch.float32, device=gz.device)
    _lib._check(_lib.load().fgnn_sage_grad_prep(_ptr(gz), gz.stride(0), _ptr(inv), _ptr(gh), _ptr(gagg), num_dst, num_src,
                                                din, _st(gz)), "fgnn_sage_grad_prep")
    return gh, gagg


class _ReluDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, d_step, tag):
        x = x.contiguous()
        y = torch.empty_like(x)
        _lib._check(_lib.load().fgnn_relu_dropout(_ptr(x), _ptr(y), x.numel(), p, seed, _ptr(d_step), tag, _st(x)),
                    "fgnn_relu_dropout")
        ctx.save_for_backward(y)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(gy)
        _lib._check(_lib.load().fgnn_relu_dropout_backward(_ptr(y), _ptr(gy), _ptr(gx), y.numel(), ctx.p, _st(y)),
                    "fgnn_relu_dropout_backward")
        return gx, None, None, None, None


def relu_dropout(x, p, training, seed=0x5A4D47, d_step=None, tag=0):
    """dropout(relu(x), p) as one launch (and one in the backward pass).  The mask comes from Philox keyed by (seed,
    *d_step, tag, element): d_step = an fgnn_hip.nn.Adam's `.step_count` (device, advanced once per step) makes every
    training step draw a fresh mask inside a replayed graph; without it the caller varies `seed`.  Eval mode, CPU
    tensors and sizes that are not a multiple of 4 take the torch ops."""
    if not training or p <= 0.0:
        return torch.relu(x)
    if not (x.is_cuda and x.dtype == torch.float32 and x.numel() % 4 == 0):
        return torch.nn.functional.dropout(torch.relu(x), p, True)
    return _ReluDropout.apply(x, float(p), int(seed), d_step, int(tag))


# ---- fused GCN / PinSAGE layers (csrc/gnn_layers.hip; the scaled aggregation: csrc/block_aggregate.hip) -------------------

def block_degrees(row, col, num_src, num_dst, edge_weight=None, want_src=True):
    """(src_deg or None, dst_deg), fp32, one launch over the edges: src_deg[row[e]] += 1 (GraphConv's out-degrees) and
    dst_deg[col[e]] += edge_weight[e] if edge_weight is given, else 1 (in-degrees / PinSAGE's weight sums)."""
    assert row.dtype == torch.int32 and col.dtype == torch.int32
    assert row.is_contiguous() and col.is_contiguous() and row.numel() == col.numel()
    if edge_weight is not None:
        assert edge_weight.dtype == torch.float32 and edge_weight.is_contiguous() and edge_weight.numel() == col.numel()
    # both vectors out of one zeroed buffer: one fill
    buf = torch.zeros((num_src if want_src else 0) + num_dst, dtype=torch.float32, device=col.device)
    src_deg, dst_deg = (buf[:num_src], buf[num_src:]) if want_src else (None, buf)
    _lib._check(_lib.load().fgnn_block_degrees(_ptr(row), _ptr(col), _ptr(edge_weight), col.numel(), _ptr(src_deg),
                                               _ptr(dst_deg), _st(col)), "fgnn_block_degrees")
    return src_deg, dst_deg


def aggregate_scaled_into(out, h, src_idx, dst_idx, edge_weight=None, src_deg=None, src_mode=0, dst_deg=None, dst_mode=0):
    """out[dst_idx[e]] += f_dst(dst_deg[dst_idx[e]]) * edge_weight[e] * f_src(src_deg[src_idx[e]]) * h[src_idx[e]] into a
    caller-initialised fp32 tensor, no autograd (modes: 0 factor 1, 1 rsqrt(max(d, 1)), 2 1 / max(d, 1)).  `out` AND `h`
    may be column blocks of wider row-major matrices (unit stride inside a row).  The backward pass of a layer is the
    same call with the index tensors, the degree vectors and the modes swapped.  h: fp32, or fp16 rows that are upcast
    on load."""
    assert h.dtype in (torch.float32, torch.float16) and out.dtype == torch.float32
    assert h.dim() == 2 and h.stride(1) == 1 and out.dim() == 2 and out.stride(1) == 1 and out.shape[1] == h.shape[1]
    assert src_idx.dtype == torch.int32 and dst_idx.dtype == torch.int32
    assert src_idx.is_contiguous() and dst_idx.is_contiguous() and src_idx.numel() == dst_idx.numel()
    for t in (edge_weight, src_deg, dst_deg):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    return _aggregate(out, h, src_idx, dst_idx, edge_weight, scaling=(src_deg, src_mode, dst_deg, dst_mode))


# ---- aggregation over whole CSR rows: exact layer-wise inference (csrc/csr_aggregate.hip; examples/inference.py) ---------

_CSR_WS = {}


def _csr_ws(device, nbytes):
    """a workspace of the CSR kernels, cached per (device, bytes)"""
    key = (torch.device(device), nbytes)
    ws = _CSR_WS.get(key)
    if ws is None:
        ws = _CSR_WS[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return ws


def csr_split_length():
    """edges of a piece: CSR rows longer than this are cut up and summed by several waves (fgnn_csr_split_length)"""
    return int(_lib.load().fgnn_csr_split_length())


def csr_workspace(device, num_rows, max_edges, dim):
    """the scratch of fgnn_csr_aggregate for these sizes on `device` (hub queue, piece descriptors, partial rows), cached
    per (device, bytes) like gat_workspace; the call expects nothing of its contents.  Calls that run concurrently on
    different streams need workspaces of their own."""
    nbytes = _lib.load().fgnn_csr_aggregate_workspace_bytes(num_rows, max_edges, dim)
    return _csr_ws(device, nbytes), nbytes


def csr_aggregate_into(out, h, indptr, indices, nodes=None, first=0, count=None, edge_weight=None, src_deg=None,
                       src_mode=0, dst_deg=None, dst_mode=0, max_edges=None):
    """out[i] = f_dst(v) * sum over v's CSR row of edge_weight[p] * f_src(indices[p]) * h[indices[p]] for v = nodes[i], or
    v = first + i for i < count (default: out's rows): fgnn_csr_aggregate, no autograd.  out (fp32) is OVERWRITTEN --
    no zero fill, rows without a neighbour become zeros --, h is fp32 or fp16 (upcast on load); both may be column blocks
    of wider row-major matrices.  indptr / indices: the int32-viewed u32 CSR tensors the engine uses; edge_weight fp32
    per CSR entry; src_deg / dst_deg fp32 per NODE with the modes of aggregate_scaled_into, dst_deg=None with a
    dst_mode taking the row's own length.  No float atomics: a row's bits depend on the row alone, whatever else the
    call computes.  max_edges: upper bound of the summed lengths of the call's rows (default: the graph's edge count,
    which holds unless `nodes` repeats ids; rows beyond the bound are still right, only summed by one wave each)."""
    assert h.dtype in (torch.float32, torch.float16) and out.dtype == torch.float32
    assert h.dim() == 2 and h.stride(1) == 1 and out.dim() == 2 and out.stride(1) == 1 and out.shape[1] == h.shape[1]
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert indptr.is_contiguous() and indices.is_contiguous()
    for t in (edge_weight, src_deg, dst_deg):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    assert edge_weight is None or edge_weight.numel() == indices.numel()
    if nodes is not None:
        assert nodes.dtype == torch.int32 and nodes.is_contiguous() and count is None
        count = nodes.numel()
    elif count is None:
        count = out.shape[0]
    assert out.shape[0] >= count and (nodes is not None or first + count <= indptr.numel() - 1)
    _lib._need_gpu(out, h, indptr, indices, nodes, edge_weight, src_deg, dst_deg)
    dim = h.shape[1]
    if max_edges is None:
        max_edges = indices.numel()
    ws, nbytes = csr_workspace(h.device, count, max_edges, dim)
    what = "fgnn_csr_aggregate" + ("_f16" if h.dtype == torch.float16 else "")
    code = getattr(_lib.load(), what)(_ptr(indptr), _ptr(indices), _ptr(edge_weight), _ptr(nodes), first, count,
                                      max_edges, _ptr(h), h.stride(0), dim, _ptr(out), out.stride(0), _ptr(src_deg),
                                      src_mode, _ptr(dst_deg), dst_mode, _ptr(ws), nbytes, _st(h))
    _lib._check(code, what)
    return out


class _ReluL2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        rows, dim = x.shape
        out = torch.empty((rows, dim), dtype=torch.float32, device=x.device)
        inv = torch.empty(rows, dtype=torch.float32, device=x.device)
        _lib._check(_lib.load().fgnn_relu_l2norm(_ptr(x), x.stride(0), _ptr(out), dim, _ptr(inv), rows, dim, _st(x)),
                    "fgnn_relu_l2norm")
        ctx.save_for_backward(out, inv)
        return out

    @staticmethod
    def backward(ctx, gout):
        out, inv = ctx.saved_tensors
        if gout.stride(1) != 1 or gout.stride(0) < gout.shape[1]:
            gout = gout.contiguous()
        rows, dim = out.shape
        gx = torch.empty_like(out)
        _lib._check(_lib.load().fgnn_relu_l2norm_backward(_ptr(out), dim, _ptr(inv), _ptr(gout), gout.stride(0), _ptr(gx),
                                                          dim, rows, dim, _st(out)), "fgnn_relu_l2norm_backward")
        return gx


def relu_l2norm(x):
    """z = relu(x); z / where(||z|| == 0, 1, ||z||) row by row as one launch (and one in the backward pass); x fp32
    [rows, dim] with unit stride inside a row."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return _ReluL2Norm.apply(x)


# ---- fused GAT layer: edge-softmax attention + aggregation (csrc/gat_attention.hip) ---------------------------------------

_GAT_WS = {}


def gat_workspace(device, num_edge, num_dst, num_head):
    """the scratch of fgnn_gat_forward / fgnn_gat_backward for these sizes on `device` (per-destination max and sums,
    per-edge scores), cached per (device, sizes): call it BEFORE a graph capture whose first gat_attention call would
    otherwise allocate it inside the capture.  Neither call expects anything of its contents."""
    key = (torch.device(device), num_edge, num_dst, num_head)
    ws = _GAT_WS.get(key)
    if ws is None:
        nbytes = _lib.load().fgnn_gat_workspace_bytes(num_edge, num_dst, num_head)
        ws = _GAT_WS[key] = torch.empty(max((nbytes + 3) // 4, 1), dtype=torch.float32, device=device)
    return ws


def _rows_ok(t):
    """[rows, H, F] fp32 with unit strides inside a row (a column block of a wider matrix is fine)"""
    return t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2] \
        and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1] * t.shape[2])


def gat_forward_into(out, alpha, feat, el, er, row, col, negative_slope=0.2, attn_p=0.0, seed=0, d_step=None, tag=0):
    """fgnn_gat_forward, no autograd: alpha [E, H] is written, the attention-weighted sums are ADDED to the
    caller-initialised out [num_dst, H, F] (out and feat may be column blocks of wider matrices)"""
    num_dst, H, F = out.shape
    assert _rows_ok(out) and _rows_ok(feat) and feat.shape[1:] == out.shape[1:]
    assert el.dtype == torch.float32 and el.is_contiguous() and el.shape == (feat.shape[0], H)
    assert er.dtype == torch.float32 and er.is_contiguous() and er.shape == (num_dst, H)
    assert row.dtype == torch.int32 and col.dtype == torch.int32 and row.is_contiguous() and col.is_contiguous()
    assert row.numel() == col.numel() and alpha.dtype == torch.float32 and alpha.is_contiguous()
    assert alpha.shape == (row.numel(), H)
    E = row.numel()
    ws = gat_workspace(feat.device, E, num_dst, H)
    _lib._check(_lib.load().fgnn_gat_forward(_ptr(row), _ptr(col), E, _ptr(el), _ptr(er), _ptr(feat), feat.stride(0),
                                             num_dst, H, F, negative_slope, attn_p, seed, _ptr(d_step), tag, _ptr(alpha),
                                             _ptr(out), out.stride(0), _ptr(ws), ws.numel() * 4, _st(feat)),
                "fgnn_gat_forward")
    return out


def gat_backward_into(gfeat, gel, ger, gout, alpha, feat, el, er, row, col, negative_slope=0.2, attn_p=0.0, seed=0,
                      d_step=None, tag=0):
    """fgnn_gat_backward, no autograd: the gradients are ADDED to the caller-initialised gfeat [num_src, H, F], gel
    [num_src, H] and ger [num_dst, H]; each may be None and is then skipped.  The dropout key is the forward call's."""
    num_dst, H, F = gout.shape
    assert _rows_ok(gout) and _rows_ok(feat) and feat.shape[1:] == gout.shape[1:]
    assert gfeat is None or (_rows_ok(gfeat) and gfeat.shape == feat.shape)
    for t, n in ((el, feat.shape[0]), (er, num_dst), (gel, feat.shape[0]), (ger, num_dst), (alpha, row.numel())):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == (n, H))
    assert row.dtype == torch.int32 and col.dtype == torch.int32 and row.is_contiguous() and col.is_contiguous()
    assert row.numel() == col.numel()
    E = row.numel()
    ws = gat_workspace(feat.device, E, num_dst, H)
    _lib._check(_lib.load().fgnn_gat_backward(_ptr(row), _ptr(col), E, _ptr(el), _ptr(er), _ptr(feat), feat.stride(0),
                                              _ptr(alpha), _ptr(gout), gout.stride(0), num_dst, H, F, negative_slope,
                                              attn_p, seed, _ptr(d_step), tag, _ptr(gfeat),
                                              gfeat.stride(0) if gfeat is not None else 0, _ptr(gel), _ptr(ger), _ptr(ws),
                                              ws.numel() * 4, _st(feat)), "fgnn_gat_backward")


class _GatAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, el, er, out, row, col, slope, attn_p, seed, d_step, tag):
        el, er = el.contiguous(), er.contiguous()
        if not _rows_ok(feat):
            feat = feat.contiguous()
        ctx.mark_dirty(out)
        alpha = torch.empty((row.numel(), feat.shape[1]), dtype=torch.float32, device=feat.device)
        gat_forward_into(out, alpha, feat, el, er, row, col, slope, attn_p, seed, d_step, tag)
        ctx.save_for_backward(feat, el, er, alpha, row, col)
        ctx.key = (slope, attn_p, seed, d_step, tag)
        return out

    @staticmethod
    def backward(ctx, gout):
        feat, el, er, alpha, row, col = ctx.saved_tensors
        if not _rows_ok(gout):
            gout = gout.contiguous()
        want = ctx.needs_input_grad
        gfeat, gel, ger = (torch.zeros_like(t, memory_format=torch.contiguous_format) if w else None
                           for t, w in zip((feat, el, er), want[:3]))
        if any(want[:3]):
            gat_backward_into(gfeat, gel, ger, gout, alpha, feat, el, er, row, col, *ctx.key)
        return gfeat, gel, ger, (gout if want[3] else None), None, None, None, None, None, None, None


def gat_attention(feat, el, er, row, col, num_dst, negative_slope=0.2, attn_drop=0.0, training=False, seed=0x5A4D47,
                  d_step=None, tag=0, out=None):
    """GAT's message passing on a block as one autograd node, differentiable in feat, el and er:
        a = edge_softmax(leaky_relu(el[row] + er[col], negative_slope)) per destination and head
        out[col[e], h, :] += dropout(a, attn_drop)[e, h] * feat[row[e], h, :]
    feat fp32 [num_src, H, F], el [num_src, H], er [num_dst, H], row / col int32 [E].  Returns [num_dst, H, F]: `out` if
    given -- a contiguous fp32 tensor that already holds what the sums are added to (a bias, a residual; gradients flow
    into it unchanged) and is modified in place -- else a new tensor.  The dropout mask (training and attn_drop > 0) comes
    from Philox keyed (seed, *d_step, tag, e H + h), see relu_dropout; the backward pass regenerates it."""
    assert feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 3
    H, F = feat.shape[1], feat.shape[2]
    assert el.dtype == torch.float32 and er.dtype == torch.float32
    assert el.shape == (feat.shape[0], H) and er.shape == (num_dst, H)
    assert row.dtype == torch.int32 and col.dtype == torch.int32
    assert row.is_contiguous() and col.is_contiguous() and row.numel() == col.numel()
    assert 0.0 <= attn_drop < 1.0
    if out is None:
        out = torch.zeros((num_dst, H, F), dtype=torch.float32, device=feat.device)
    assert out.dtype == torch.float32 and out.shape == (num_dst, H, F) and out.is_contiguous()
    p = float(attn_drop) if training else 0.0
    return _GatAttention.apply(feat, el, er, out, row, col, float(negative_slope), p, int(seed), d_step, int(tag))


# ---- GAT attention over whole CSR rows: exact layer-wise GAT inference (csrc/csr_gat_attention.hip) ---------------------

def csr_gat_max_heads():
    """heads the kernel's per-wave staging of the edge weights holds (fgnn_csr_gat_max_heads); more are refused"""
    return int(_lib.load().fgnn_csr_gat_max_heads())


def csr_gat_workspace(device, num_rows, max_edges, H, F):
    """the scratch of fgnn_csr_gat_attention for these sizes on `device` (hub queue, piece descriptors, partial rows),
    cached per (device, bytes) together with csr_workspace's; the call expects nothing of its contents.  Calls that run
    concurrently on different streams need workspaces of their own."""
    nbytes = _lib.load().fgnn_csr_gat_workspace_bytes(num_rows, max_edges, H, F)
    return _csr_ws(device, nbytes), nbytes


def csr_gat_attention_into(out, feat, el, er, indptr, indices, nodes=None, first=0, count=None, negative_slope=0.2,
                           max_edges=None):
    """out[i, h, :] = sum over v's CSR row of a[p, h] * feat[indices[p], h, :] with a[., h] = softmax over the row of
    leaky_relu(el[indices[p], h] + er[v, h], negative_slope), for v = nodes[i], or v = first + i for i < count (default:
    out's rows): fgnn_csr_gat_attention, no autograd, no dropout.  out [rows, H, F] (fp32) is OVERWRITTEN -- no zero
    fill, rows without a neighbour become zeros --, feat is [N, H, F] fp32; both may be column blocks of wider row-major
    matrices.  el and er are fp32 [N, H], one row per NODE (er too, unlike gat_forward_into's).  indptr / indices: the
    int32-viewed u32 CSR tensors the engine uses.  No float atomics: a row's bits depend on the row alone, whatever
    else the call computes.  H <= csr_gat_max_heads().  max_edges: upper bound of the summed lengths of the call's rows
    (default: the graph's edge count, which holds unless `nodes` repeats ids; rows beyond the bound are still right,
    only computed by one wave each)."""
    assert _rows_ok(out) and _rows_ok(feat) and feat.shape[1:] == out.shape[1:]
    N, H, F = feat.shape
    assert el.dtype == torch.float32 and el.is_contiguous() and el.shape == (N, H)
    assert er.dtype == torch.float32 and er.is_contiguous() and er.shape == (N, H)
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert indptr.is_contiguous() and indices.is_contiguous()
    if nodes is not None:
        assert nodes.dtype == torch.int32 and nodes.is_contiguous() and count is None
        count = nodes.numel()
    elif count is None:
        count = out.shape[0]
    assert out.shape[0] >= count and (nodes is not None or first + count <= indptr.numel() - 1)
    _lib._need_gpu(out, feat, el, er, indptr, indices, nodes)
    if max_edges is None:
        max_edges = indices.numel()
    ws, nbytes = csr_gat_workspace(feat.device, count, max_edges, H, F)
    code = _lib.load().fgnn_csr_gat_attention(_ptr(indptr), _ptr(indices), _ptr(nodes), first, count, max_edges, _ptr(el),
                                              _ptr(er), _ptr(feat), feat.stride(0), H, F, negative_slope, _ptr(out),
                                              out.stride(0), _ptr(ws), nbytes, _st(feat))
    _lib._check(code, "fgnn_csr_gat_attention")
    return out


class _XentWs:
    """scratch of fgnn_softmax_xent per (device, n): arrival counter (zeroed once) + row losses"""
    cache = {}

    @classmethod
    def get(cls, device, n):
        key = (torch.device(device), n)
        ws = cls.cache.get(key)
        if ws is None:
            nbytes = _lib.load().fgnn_softmax_xent_scratch_bytes(n)
            ws = cls.cache[key] = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)
        return ws


def xent_scratch(device, n):
    """creates the scratch softmax_xent uses for n rows on `device` (arrival counter zeroed once + partial sums): call
    it BEFORE a graph capture whose first softmax_xent call would otherwise allocate -- and zero -- it inside the
    capture (a memset node in every replay, a buffer of the graph's private pool in this module's cache)"""
    return _XentWs.get(torch.device(device), n)


_XENT_GRAD = {}


def xent_grad_buffer(device, rows, num_class):
    """the reusable, zero-initialised gradient buffer softmax_xent(..., pad_rows) hands out for this shape: create it
    BEFORE a graph capture that will use it (an allocation inside a capture belongs to that graph's pool and its
    zeroing would be replayed)"""
    key = (torch.device(device), rows, num_class)
    g = _XENT_GRAD.get(key)
    if g is None:
        g = _XENT_GRAD[key] = torch.zeros((rows, num_class), dtype=torch.float32, device=device)
    return g


def softmax_xent(logits, labels, pad_rows=0):
    """(loss, dlogits): CrossEntropyLoss(reduction='mean')(logits, labels) and d loss / d logits, one launch.  Use as
    `loss, g = softmax_xent(out, y); out.backward(g)`: no scalar multiply node between the loss and the first GEMM.
    pad_rows > 0: dlogits has that many extra all-zero rows behind the n real ones (the gradient of a padded output
    whose first n rows carry the loss -- no zeros + slice-backward pair) and lives in a buffer that is reused by the
    next call with the same shape: consume it (backward) before calling again."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == logits.shape[0]
    n, c = logits.shape
    ws = _XentWs.get(logits.device, n)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    if pad_rows:
        g = xent_grad_buffer(logits.device, n + pad_rows, c)
    else:
        g = torch.empty((n, c), dtype=torch.float32, device=logits.device)
    _lib._check(_lib.load().fgnn_softmax_xent(_ptr(logits), logits.stride(0), _ptr(labels), n, c, _ptr(loss), _ptr(g), c,
                                              _ptr(ws), ws.numel() * 4, _st(logits)), "fgnn_softmax_xent")
    return loss, g


class Adam:
    """torch.optim.Adam's update (lr, betas, eps, weight_decay; no amsgrad) for a handful of fp32 tensors as ONE launch
    per step, the step count on the device (`step_count`: two int64 words) -- capturable by construction.  The
    interface the training loops use: zero_grad(set_to_none=True), step(), param_groups[0]['lr'], state_dict()."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.params = [p for p in params if p.requires_grad]
        assert self.params and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in self.params)
        dev = self.params[0].device
        self.param_groups = [dict(params=self.params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.step_count = torch.zeros(2, dtype=torch.int64, device=dev)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def step(self):
        g = self.param_groups[0]
        L = _lib.load()
        live = [(p, m, v) for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq) if p.grad is not None]
        for a in range(0, len(live), 8):  # eight tensors per launch
            chunk = live[a:a + 8]
            k = len(chunk)
            grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p, _, _ in chunk]
            arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])  # noqa: E731
            numel = (C.c_size_t * k)(*[p.numel() for p, _, _ in chunk])
            # (only the LAST launch of a step advances the count: earlier ones get a scratch counter that starts equal)
            last = a + 8 >= len(live)
            cnt = self.step_count if last else self.step_count.clone()
            _lib._check(L.fgnn_adam_step(arr([p for p, _, _ in chunk]), arr(grads), arr([m for _, m, _ in chunk]),
                                         arr([v for _, _, v in chunk]), numel, k, g["lr"], g["betas"][0], g["betas"][1],
                                         g["eps"], g["weight_decay"], _ptr(cnt), _st(self.step_count)), "fgnn_adam_step")

    def state_dict(self):
        return {"step": int(self.step_count[0]), "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"}]}
