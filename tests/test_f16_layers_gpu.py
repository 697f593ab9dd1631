"""fp16 input features into the example models (examples/models.py): the first layer of the fused SAGE, GCN and PinSAGE
models reads the half rows as they are and must give what the same layer gives for feat.float() -- the same fp32
terms, added in an order that differs only between waves, so the tolerances are those tests/test_fused_gnn_gpu.py
derives from the aggregation bound for two evaluations of one layer (output rtol / atol 1e-4, weight and bias
gradients rtol 1e-4 / atol 2e-3).  GAT and the op-by-op layers upcast once with torch."""
import importlib
import os
import sys

import pytest
import torch

import test_fused_gnn_gpu as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSRC, NDST = T.NSRC, T.NDST


@pytest.fixture(scope="module")
def models():
    from fgnn_hip import lib
    lib.load()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    m = importlib.import_module("models")
    assert m._fused_aggregate is not None
    return m


@pytest.fixture(scope="module")
def block_edges():
    row, col, w, _ = T._make_edges()
    return row.int().cuda(), col.int().cuda(), w.int().cuda()


def _layer(models, kind, din, dout):
    torch.manual_seed(din + dout)
    if kind == "sage":
        return models.FusedSAGEConv(din, dout).cuda()
    if kind == "gcn":
        return models.FusedGraphConv(din, dout).cuda()
    return models.FusedWeightedSAGEConv(din, 48, dout, 0.0).cuda()


def _run(layer, blk, x, gy):
    layer.zero_grad()
    y = layer(blk, x)
    y.backward(gy)
    return y.detach(), {k: p.grad.clone() for k, p in layer.named_parameters()}


def _close(got, want):
    torch.testing.assert_close(got[0], want[0], rtol=1e-4, atol=1e-4)
    assert sorted(got[1]) == sorted(want[1])
    for k in got[1]:
        torch.testing.assert_close(got[1][k], want[1][k], rtol=1e-4, atol=2e-3)


def _inputs(din, dout):
    g = torch.Generator(device="cuda").manual_seed(din)
    x16 = torch.randn((NSRC, din), device="cuda", generator=g).half()
    return x16, torch.randn((NDST, dout), device="cuda", generator=g)


@pytest.mark.parametrize("kind", ["sage", "gcn", "pinsage"])
@pytest.mark.parametrize("din,dout", [(96, 64), (100, 47), (77, 16)])
def test_first_layer_reads_half_rows_like_the_upcast_rows(models, block_edges, kind, din, dout):
    """din 96: two columns per lane and fgnn_sage_finish_z_f16; 100: two columns per lane, din % 4 == 0; 77: odd, one
    column per lane and the torch copy of the destinations' rows"""
    row, col, w = block_edges
    blk = T.Block(row, col, NDST, w if kind == "pinsage" else None)
    layer = _layer(models, kind, din, dout)
    x16, gy = _inputs(din, dout)
    assert models._half_rows_apply(blk, x16) and models.input_rows(layer, blk, x16) is x16
    got = _run(layer, blk, x16, gy)
    assert got[0].dtype == torch.float32 and bool(got[0].abs().sum() > 0)
    _close(got, _run(layer, blk, x16.float(), gy))


@pytest.mark.parametrize("kind", ["sage", "gcn", "pinsage"])
def test_half_first_layer_captures_into_a_graph(models, block_edges, kind):
    """forward + backward with an fp16 input placeholder: nothing synchronises, the replay computes the eager result"""
    row, col, w = block_edges
    blk = T.Block(row, col, NDST, w if kind == "pinsage" else None)
    layer = _layer(models, kind, 96, 64)
    x0, gy = _inputs(96, 64)
    want = _run(layer, blk, x0, gy)  # eager warm-up
    layer.zero_grad()
    x = torch.zeros_like(x0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = layer(blk, x)
        y.backward(gy)
    x.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    _close((y.detach(), {k: p.grad for k, p in layer.named_parameters()}), want)


@pytest.mark.parametrize("kind,fused", [("graphsage", True), ("gcn", True), ("pinsage", True), ("gat", True),
                                        ("graphsage", False), ("gcn", False)])
def test_models_take_half_features(models, block_edges, kind, fused):
    """whole models, eval mode: fp16 features against the same features upcast by the caller.  The fused SAGE / GCN /
    PinSAGE models hand the half tensor to their first layer; GAT and the op-by-op models upcast it themselves."""
    row, col, w = block_edges
    blocks = [T.Block(row, col, NDST, w)]
    g = torch.Generator().manual_seed(31)
    r = torch.randint(0, NDST, (901,), generator=g).int().cuda()
    c = torch.sort(torch.randint(0, 59, (901,), generator=g))[0].int().cuda()
    blocks.append(T.Block(r, c, 60, torch.randint(1, 9, (901,), generator=g).int().cuda()))
    torch.manual_seed(9)
    m = models.MODELS[kind](96, 64, 10, 2, 0.0, fused=fused).cuda().eval()
    x16, _ = _inputs(96, 64)
    first = models.input_rows(m.layers[0], blocks[0], x16)
    assert (first is x16) == (fused and kind != "gat") and (first is x16 or first.dtype == torch.float32)
    with torch.no_grad():
        a, b = m(blocks, x16), m(blocks, x16.float())
    assert a.dtype == torch.float32 and a.shape == (60, 10)
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
