"""The fused GCN / PinSAGE layers on the GPU: the four kernels of csrc/gnn_layers.hip against plain torch fp32, the
layers and models of examples/models.py against their op-by-op counterparts, and the capture contract (no host
synchronisation anywhere in a layer's forward + backward).

One small block serves every test: E = 6001 edges (no multiple of the 32 edges a wave takes), 2000 sources, 300
destinations; a destination with > 100 edges whose run crosses a workgroup boundary of both edge kernels, 7
destinations and 100 sources without an edge (the max(d, 1) clamps), a source referenced > 100 times."""
import ctypes as C
import importlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NSRC, NDST = 6001, 2000, 300
NO_EDGE_DST = (0, 17, 101, 150, 222, 298, 299)
HUB_SRC = 5


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


@pytest.fixture(scope="module")
def models(hip):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    m = importlib.import_module("models")
    assert m._fused_aggregate is not None
    return m


class Block:
    def __init__(self, row, col, ndst, w=None):
        self.row, self.col, self.ndst = row, col, ndst
        self.edata = {"weights": w} if w is not None else {}

    def number_of_dst_nodes(self):
        return self.ndst


def _make_edges():
    g = torch.Generator().manual_seed(77)
    allowed = torch.tensor([d for d in range(NDST) if d not in NO_EDGE_DST])
    col = torch.sort(allowed[torch.randint(0, len(allowed), (E - 150,), generator=g)])[0]
    hub = int(col[2485])  # its run will cover edge 2560 = 10 * 256 = 20 * 128
    col = torch.sort(torch.cat([col, torch.full((150,), hub)]))[0]
    run = (col == hub).nonzero().flatten()
    assert len(run) >= 150 and int(run[0]) < 2560 <= int(run[-1])
    row = torch.randint(0, NSRC - 100, (E,), generator=g)  # the last 100 sources have no edge
    row[torch.randperm(E, generator=g)[:120]] = HUB_SRC
    w = torch.randint(1, 9, (E,), generator=g)
    perm = torch.randperm(E, generator=g)
    return row, col, w, perm


@pytest.fixture(scope="module")
def edges(hip):
    """{'sorted' | 'unsorted'}: (row int32, col int32, w fp32 with integer values 1..8) on the GPU"""
    row, col, w, perm = _make_edges()
    out = {}
    for name, idx in (("sorted", torch.arange(E)), ("unsorted", perm)):
        out[name] = (row[idx].int().cuda(), col[idx].int().cuda(), w[idx].float().cuda())
    return out


def _counts(idx, n, weights=None):
    return torch.bincount(idx.long(), weights=weights, minlength=n).float()


# ---- fgnn_block_degrees -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["sorted", "unsorted"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("want_src", [True, False])
def test_block_degrees_equal_bincount_exactly(hip, edges, order, weighted, want_src):
    """integer-valued fp32 sums below 2^24 are exact in any order: equality, not a tolerance"""
    from fgnn_hip.nn import block_degrees
    row, col, w = edges[order]
    src_deg, dst_deg = block_degrees(row, col, NSRC, NDST, edge_weight=w if weighted else None, want_src=want_src)
    assert torch.equal(dst_deg, _counts(col, NDST, w.double() if weighted else None))
    assert not dst_deg[list(NO_EDGE_DST)].any() and float(dst_deg.max()) >= 150
    if want_src:
        assert torch.equal(src_deg, _counts(row, NSRC))
        assert float(src_deg[HUB_SRC]) >= 120 and not src_deg[NSRC - 100:].any()
    else:
        assert src_deg is None


def test_block_degrees_of_an_empty_block_are_zero(hip):
    from fgnn_hip.nn import block_degrees
    e = torch.empty(0, dtype=torch.int32, device="cuda")
    src_deg, dst_deg = block_degrees(e, e, 9, 4)
    assert src_deg.shape == (9,) and dst_deg.shape == (4,) and not src_deg.any() and not dst_deg.any()
    _, dst_deg = block_degrees(e, e, 9, 4, edge_weight=torch.empty(0, device="cuda"), want_src=False)
    assert not dst_deg.any()


# ---- fgnn_block_aggregate_scaled -----------------------------------------------------------------------------------------

def _factor(d, mode):
    d = d.clamp(min=1)
    return torch.ones_like(d) if mode == 0 else (d.pow(-0.5) if mode == 1 else 1.0 / d)


AGG_CASES = [(dim, modes, weighted, "sorted") for dim in (256, 100, 64, 7) for modes in ((0, 0), (1, 1), (0, 2), (2, 0))
             for weighted in (False, True)] + [(100, modes, True, "unsorted") for modes in ((1, 1), (0, 2))]


@pytest.mark.parametrize("dim,modes,weighted,order", AGG_CASES)
def test_aggregate_scaled_matches_torch_reference(hip, edges, dim, modes, weighted, order):
    """against out.index_add_(0, col, w f_src h[row]) * f_dst in torch fp32; rtol / atol 1e-4, the tolerance of
    fgnn_block_aggregate's own test (the order of the float additions differs).  h and out are column blocks of wider
    matrices; what lies beside the output block must not change by a bit."""
    from fgnn_hip.nn import aggregate_into, aggregate_scaled_into
    row, col, w = edges[order]
    w = w if weighted else None
    src_mode, dst_mode = modes
    g = torch.Generator(device="cuda").manual_seed(dim)
    hbig = torch.randn((NSRC, dim + 13), device="cuda", generator=g)
    h = hbig[:, 5:5 + dim]
    obig = torch.randn((NDST, dim + 24), device="cuda", generator=g)
    obig[:, 8:8 + dim] = 0
    before = obig.clone()
    src_deg = _counts(row, NSRC)
    dst_deg = _counts(col, NDST, w.double() if weighted else None)
    out = aggregate_scaled_into(obig[:, 8:8 + dim], h, row, col, w, src_deg if src_mode else None, src_mode,
                                dst_deg if dst_mode else None, dst_mode)
    msg = h[row.long()] * _factor(src_deg, src_mode)[row.long()].unsqueeze(1)
    if weighted:
        msg = msg * w.unsqueeze(1)
    ref = torch.zeros((NDST, dim), device="cuda").index_add_(0, col.long(), msg) * _factor(dst_deg, dst_mode).unsqueeze(1)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(obig[:, :8], before[:, :8]) and torch.equal(obig[:, 8 + dim:], before[:, 8 + dim:])
    assert not out[list(NO_EDGE_DST)].any()
    if modes == (0, 0) and not weighted:
        plain = aggregate_into(torch.zeros((NDST, dim), device="cuda"), h.contiguous(), row, col)
        torch.testing.assert_close(out, plain, rtol=1e-4, atol=1e-4)


def test_aggregate_scaled_refuses_bad_arguments_without_a_launch(hip, edges):
    from fgnn_hip.nn import aggregate_scaled_into
    row, col, _ = edges["sorted"]
    L = hip.load()
    h = torch.ones((NSRC, 8), device="cuda")
    out = torch.zeros((NDST, 8), device="cuda")
    deg = torch.ones(NSRC, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(out_ptr=out.data_ptr(), dim=8, out_ld=8, src_mode=0, dst_mode=0):
        return L.fgnn_block_aggregate_scaled(C.c_void_p(row.data_ptr()), C.c_void_p(col.data_ptr()), None, C.c_size_t(E),
                                             C.c_void_p(h.data_ptr()), C.c_size_t(8), C.c_size_t(dim),
                                             C.c_void_p(out_ptr), C.c_size_t(out_ld), C.c_void_p(deg.data_ptr()),
                                             C.c_int(src_mode), C.c_void_p(deg.data_ptr()), C.c_int(dst_mode), st)

    for bad in (dict(out_ptr=None), dict(dim=0), dict(out_ld=7), dict(src_mode=3), dict(dst_mode=-1),
                dict(out_ptr=out.data_ptr() + 2)):
        code = call(**bad)
        assert code == -1, (bad, code)  # FGNN_EINVAL
        with pytest.raises(hip.FgnnError):
            hip._check(code, "fgnn_block_aggregate_scaled")
    with pytest.raises(hip.FgnnError):
        aggregate_scaled_into(out, h, row, col, None, deg, 3, None, 0)
    with pytest.raises(hip.FgnnError):  # a mode without its degree vector
        aggregate_scaled_into(out, h, row, col, None, None, 1, None, 0)
    # the plain entry points go through the same checks: a pointer that is not 4-byte aligned launches nothing
    for where in range(5):
        ptrs = [row.data_ptr(), col.data_ptr(), h.data_ptr(), out.data_ptr(), deg.data_ptr()]
        ptrs[where] += 2
        assert L.fgnn_block_aggregate_ex(C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), None, C.c_size_t(E), C.c_void_p(ptrs[2]),
                                         C.c_size_t(8), C.c_void_p(ptrs[3]), C.c_size_t(8), C.c_void_p(ptrs[4]), st) == -1
    assert L.fgnn_block_aggregate(C.c_void_p(row.data_ptr()), C.c_void_p(col.data_ptr()), None, C.c_size_t(E),
                                  C.c_void_p(h.data_ptr()), C.c_size_t(8), C.c_void_p(out.data_ptr() + 2), st) == -1
    torch.cuda.synchronize()
    assert bool((deg == 1).all())
    assert not out.any()  # nothing was launched
    assert call() == 0 and bool(out.any())
    # a zero size is fine and launches nothing, whatever else is passed
    assert L.fgnn_block_aggregate_scaled(None, None, None, C.c_size_t(0), None, C.c_size_t(0), C.c_size_t(0), None,
                                         C.c_size_t(0), None, C.c_int(0), None, C.c_int(0), st) == 0
    x = torch.ones((4, 8), device="cuda")
    inv = torch.zeros(4, device="cuda")
    for rows, dim, ld in ((4, 0, 8), (4, 8, 7)):
        assert L.fgnn_relu_l2norm(C.c_void_p(x.data_ptr()), C.c_size_t(ld), C.c_void_p(out.data_ptr()), C.c_size_t(8),
                                  C.c_void_p(inv.data_ptr()), C.c_size_t(rows), C.c_size_t(dim), st) == -1
    assert L.fgnn_relu_l2norm(None, C.c_size_t(8), None, C.c_size_t(8), None, C.c_size_t(0), C.c_size_t(8), st) == 0
    assert L.fgnn_block_degrees(None, C.c_void_p(col.data_ptr()), None, C.c_size_t(E), None, None, st) == -1


# ---- fgnn_relu_l2norm -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [256, 150, 7, 1, 300])
def test_relu_l2norm_matches_torch_under_autograd(hip, dim):
    """forward and input gradient against z = relu(x); z / where(norm == 0, 1, norm); rtol 1e-4, atol 1e-5.  Every tenth
    row has no positive entry (zero norm): exactly 0 out, exactly 0 gradient.  The input is a column block of a wider
    matrix.  |x| >= 0.25 everywhere: the gradient's rounding error scales with 1 / norm, and a row of one or seven
    entries can otherwise have a norm of 1e-3 -- then the two formulations' fp32 results lie 1e-4 apart although both
    are right (dim 300: wider than the 256 columns a wave keeps in registers)."""
    from fgnn_hip.nn import relu_l2norm
    rows = 513
    g = torch.Generator(device="cuda").manual_seed(100 + dim)
    big = torch.randn((rows, dim + 9), device="cuda", generator=g)
    big = big + 0.25 * torch.sign(big)
    big[::10] = -big[::10].abs()
    gout = torch.randn((rows, dim), device="cuda", generator=g)
    res = []
    for fused in (True, False):
        b = big.clone().requires_grad_()
        x = b[:, 3:3 + dim]
        if fused:
            y = relu_l2norm(x)
        else:
            z = torch.relu(x)
            n = z.norm(2, 1, keepdim=True)
            y = z / torch.where(n == 0, torch.ones_like(n), n)
        y.backward(gout)
        res.append((y.detach(), b.grad))
    torch.testing.assert_close(res[0][0], res[1][0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-4, atol=1e-5)
    assert not res[0][0][::10].any() and not res[0][1][::10].any()
    assert bool(res[0][0][1].any())


# ---- layers ------------------------------------------------------------------------------------------------------------------

def _layer_pair(models, kind, din, dout):
    torch.manual_seed(din)
    if kind == "gcn":
        fused, plain = models.FusedGraphConv(din, dout), models.GraphConv(din, dout)
    else:
        fused, plain = models.FusedWeightedSAGEConv(din, 48, dout, 0.0), models.WeightedSAGEConv(din, 48, dout, 0.0)
    plain.load_state_dict(fused.state_dict(), strict=True)
    fused.load_state_dict(plain.state_dict(), strict=True)
    return fused.cuda(), plain.cuda()


def _run_layer(layer, blk, x, gy, need_gh):
    layer.zero_grad()
    h = x.clone().requires_grad_(need_gh)
    y = layer(blk, h)
    y.backward(gy)
    return y.detach(), (h.grad if need_gh else None), {k: p.grad.clone() for k, p in layer.named_parameters()}


def _check_layer(got, want, need_gh):
    torch.testing.assert_close(got[0], want[0], rtol=1e-4, atol=1e-4)
    if need_gh:
        torch.testing.assert_close(got[1], want[1], rtol=1e-3, atol=1e-4)
    assert sorted(got[2]) == sorted(want[2])
    for k in got[2]:
        torch.testing.assert_close(got[2][k], want[2][k], rtol=1e-4, atol=2e-3)


@pytest.mark.parametrize("kind", ["gcn", "pinsage"])
@pytest.mark.parametrize("din,dout", [(96, 64), (100, 47)])
@pytest.mark.parametrize("need_gh", [True, False])
def test_fused_layers_match_the_op_by_op_layers(hip, models, edges, kind, din, dout, need_gh):
    """output 1e-4 / 1e-4, input gradient rtol 1e-3 / atol 1e-4 (test_example_layers_same_with_fused_and_torch_
    aggregation's), weight and bias gradients rtol 1e-4 / atol 2e-3 (test_fused_sage_layer_matches_the_op_by_op_layer's);
    the op-by-op layer once with fgnn_block_aggregate and once with torch's gather + index_add_ (no kernel of this
    repository in the comparison)."""
    row, col, w = edges["sorted"]
    blk = Block(row, col, NDST, w.int() if kind == "pinsage" else None)
    fused, plain = _layer_pair(models, kind, din, dout)
    g = torch.Generator(device="cuda").manual_seed(dout)
    x = torch.randn((NSRC, din), device="cuda", generator=g)
    gy = torch.randn((NDST, dout), device="cuda", generator=g)
    got = _run_layer(fused, blk, x, gy, need_gh)
    _check_layer(got, _run_layer(plain, blk, x, gy, need_gh), need_gh)
    saved = models._fused_aggregate
    models._fused_aggregate = None
    try:
        want = _run_layer(plain, blk, x, gy, need_gh)
    finally:
        models._fused_aggregate = saved
    _check_layer(got, want, need_gh)


@pytest.mark.parametrize("kind", ["gcn", "pinsage"])
def test_fused_layer_forward_and_backward_capture_into_a_graph(hip, models, edges, kind):
    """the contract a graphed stepper will rely on: nothing in a fused layer's forward + backward synchronises with the
    host (a sync or an .item() makes the capture raise), and the replay computes what the eager pass computes"""
    row, col, w = edges["sorted"]
    blk = Block(row, col, NDST, w.int() if kind == "pinsage" else None)
    fused, _ = _layer_pair(models, kind, 96, 64)
    g = torch.Generator(device="cuda").manual_seed(8)
    x0 = torch.randn((NSRC, 96), device="cuda", generator=g)
    gy = torch.randn((NDST, 64), device="cuda", generator=g)
    want = _run_layer(fused, blk, x0, gy, True)  # eager warm-up: lazy initialisation happens here
    fused.zero_grad()
    x = torch.zeros_like(x0).requires_grad_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = fused(blk, x)
        y.backward(gy)
    with torch.no_grad():
        x.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    got = (y.detach(), x.grad, {k: p.grad for k, p in fused.named_parameters()})
    _check_layer(got, want, True)


# ---- models ------------------------------------------------------------------------------------------------------------------

def _chain(edges):
    """three blocks 2000 -> 300 -> 60 -> 12; the outer one is the common block"""
    row, col, w = edges["sorted"]
    g = torch.Generator().manual_seed(31)
    blocks = [Block(row, col, NDST, w.int())]
    for nsrc, ndst, ne in ((NDST, 60, 901), (60, 12, 100)):
        r = torch.randint(0, nsrc, (ne,), generator=g).int().cuda()
        c = torch.sort(torch.randint(0, ndst - 1, (ne,), generator=g))[0].int().cuda()
        ww = torch.randint(1, 9, (ne,), generator=g).int().cuda()
        blocks.append(Block(r, c, ndst, ww))
    return blocks


@pytest.mark.parametrize("kind", ["gcn", "pinsage"])
def test_fused_models_train_like_the_op_by_op_models(hip, models, edges, kind):
    """three Adam steps (fgnn_hip.nn.Adam, its step count keying the fused model's ReLU + dropout as the pipelines set
    it; dropout 0) from the same weights: every parameter within rtol 1e-4 / atol 1e-5, then the eval-mode outputs"""
    from fgnn_hip.nn import Adam
    blocks = _chain(edges)
    torch.manual_seed(3)
    fused = models.MODELS[kind](96, 64, 10, 3, 0.0, fused=True).cuda()
    plain = models.MODELS[kind](96, 64, 10, 3, 0.0, fused=False).cuda()
    plain.load_state_dict(fused.state_dict(), strict=True)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((NSRC, 96), device="cuda", generator=g)
    label = torch.randint(0, 10, (12,), device="cuda", generator=g)
    for m in (fused, plain):
        opt = Adam(m.parameters(), lr=0.003)
        if m is fused:
            m.dropout_step = opt.step_count
        m.train()
        for _ in range(3):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(m(blocks, x), label).backward()
            opt.step()
    for (k, p), (k2, q) in zip(fused.named_parameters(), plain.named_parameters()):
        assert k == k2
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-5, msg=lambda s, k=k: "%s: %s" % (k, s))
    fused.eval()
    plain.eval()
    with torch.no_grad():
        torch.testing.assert_close(fused(blocks, x), plain(blocks, x), rtol=1e-4, atol=1e-4)
