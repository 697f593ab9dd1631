"""q8 input features into the example models (examples/models.py): the first layer of the fused SAGE, GCN and PinSAGE
models takes the 8-bit rows as they are and must give what the op-by-op layer gives for the decoded fp32 rows -- the
aggregation bound of tests/test_q8_kernels_gpu.py carried through the linear layer the way tests/test_f16_layers_gpu.py
carries the fp32 kernels' (output rtol / atol 1e-4).  GAT and the op-by-op layers get one decode."""
import pytest
import torch

import test_fused_gnn_gpu as T
from test_f16_layers_gpu import block_edges, models  # noqa: F401  (examples/models.py and the 6001-edge block as fixtures)
from test_layerwise_inference_gpu import _model, graph  # noqa: F401  (the R-MAT graph with a hub row, the models)

pytestmark = pytest.mark.gpu
NSRC, NDST = T.NSRC, T.NDST


def _pair(models, kind, din, dout):  # noqa: F811
    """(fused layer, op-by-op layer with the same parameters)"""
    torch.manual_seed(din + dout)
    if kind == "sage":
        fused, plain = models.FusedSAGEConv(din, dout).cuda(), models.SAGEConvMean(din, dout).cuda()
        plain.load_state_dict(fused.split_state_dict())
        return fused, plain
    if kind == "gcn":
        fused, plain = models.FusedGraphConv(din, dout).cuda(), models.GraphConv(din, dout).cuda()
    else:
        fused, plain = models.FusedWeightedSAGEConv(din, 48, dout, 0.0).cuda(), models.WeightedSAGEConv(din, 48, dout, 0.0).cuda()
    plain.load_state_dict(fused.state_dict())
    return fused, plain


# din 96: one load per row, fgnn_sage_finish_z_q8; 77: din % 4 != 0, the destinations' rows by the decode kernel; 600:
# rows walked in three passes
@pytest.mark.parametrize("kind", ["sage", "gcn", "pinsage"])
@pytest.mark.parametrize("din,dout", [(96, 64), (77, 16), (600, 32)])
def test_first_layer_reads_q8_rows_like_the_op_by_op_layer_reads_the_decoded_rows(models, block_edges, kind, din, dout):  # noqa: F811
    from fgnn_hip import lib
    row, col, w = block_edges
    blk = T.Block(row, col, NDST, w if kind == "pinsage" else None)
    fused, plain = _pair(models, kind, din, dout)
    x = torch.randn((NSRC, din), device="cuda", generator=torch.Generator(device="cuda").manual_seed(din))
    rows = lib.quantize_rows_q8(x)
    decoded = lib.dequantize_rows_q8(rows, din)
    assert models._q8_rows_apply(blk, rows) and models.input_rows(fused, blk, rows) is rows
    first = models.input_rows(plain, blk, rows)
    assert first.dtype == torch.float32 and torch.equal(first, decoded)
    with torch.no_grad():
        got, want = fused(blk, rows), plain(blk, decoded)
    assert got.dtype == torch.float32 and got.shape == (NDST, dout) and bool(got.abs().sum() > 0)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("kind,fused", [("graphsage", True), ("gcn", True), ("pinsage", True), ("gat", True),
                                        ("graphsage", False)])
def test_models_take_q8_features(models, block_edges, kind, fused):  # noqa: F811
    """whole models, eval mode: q8 features against the same rows decoded by the caller; only the fused SAGE / GCN /
    PinSAGE models hand the uint8 tensor to their first layer, GAT and the op-by-op models decode it themselves"""
    from fgnn_hip import lib
    row, col, w = block_edges
    blocks = [T.Block(row, col, NDST, w)]
    g = torch.Generator().manual_seed(31)
    r = torch.randint(0, NDST, (901,), generator=g).int().cuda()
    c = torch.sort(torch.randint(0, 59, (901,), generator=g))[0].int().cuda()
    blocks.append(T.Block(r, c, 60, torch.randint(1, 9, (901,), generator=g).int().cuda()))
    torch.manual_seed(9)
    m = models.MODELS[kind](96, 64, 10, 2, 0.0, fused=fused).cuda().eval()
    rows = lib.quantize_rows_q8(torch.randn((NSRC, 96), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)))
    first = models.input_rows(m.layers[0], blocks[0], rows)
    assert (first is rows) == (fused and kind != "gat") and (first is rows or first.dtype == torch.float32)
    with torch.no_grad():
        a, b = m(blocks, rows), m(blocks, lib.dequantize_rows_q8(rows, 96))
    assert a.dtype == torch.float32 and a.shape == (60, 10)
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", ["graphsage", "gcn"])
def test_layerwise_inference_reads_a_q8_table_as_it_is(graph, name):  # noqa: F811
    """the q8 table through fgnn_csr_aggregate_q8 (hub row included) against the same pass over the decoded table"""
    from fgnn_hip import lib
    from inference import layerwise_inference
    indptr, indices, feats = graph
    model = _model(name, True, 100).cuda()
    rows = lib.quantize_rows_q8(feats[100].cuda())
    got = layerwise_inference(model, indptr, indices, rows)
    want = layerwise_inference(model, indptr, indices, lib.dequantize_rows_q8(rows, 100))
    assert got.dtype == torch.float32 and got.shape == want.shape
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
