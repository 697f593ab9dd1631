"""CPU-only: the max-pooling aggregator at every level -- entry points, layers, SAGE's `aggregator=`, exact inference."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from test_gat_exports import _Block, _tiny_blocks  # noqa: E402  (the two-block chain 12 -> 5 -> 2)

NEW = {"fgnn_block_relu_max_workspace_bytes": "size_t", "fgnn_block_relu_max_forward": "int",
       "fgnn_block_relu_max_backward": "int"}


def test_library_header_and_binding_carry_the_three_entry_points():
    from fgnn_hip import lib
    so = ctypes.CDLL(lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fgnn_hip.h")).read(), flags=re.S)
    for name, ret in NEW.items():
        assert hasattr(so, name), name
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), name
        assert name in lib.EXPORTS and name in lib.SIGNATURES, name
    ws = lib.load().fgnn_block_relu_max_workspace_bytes  # needs no GPU
    assert ws(10, 7) >= 10 * 7 * 8 and ws(11, 7) > ws(10, 7) and ws(10, 8) > ws(10, 7)


@pytest.mark.parametrize("fused", [True, False])
def test_sage_aggregator_keyword_selects_the_layers(fused):
    import models
    pool = models.SAGE(8, 8, 3, 2, 0.0, aggregator="pool", fused=fused)
    assert all(type(l) is (models.FusedSAGEPoolConv if fused else models.SAGEConvPool) for l in pool.layers)
    mean = models.SAGE(8, 8, 3, 2, 0.0, fused=fused)
    assert all(type(l) is (models.FusedSAGEConv if fused else models.SAGEConvMean) for l in mean.layers)
    with pytest.raises(ValueError):
        models.SAGE(8, 8, 3, 2, 0.0, aggregator="lstm", fused=fused)


def test_fused_pool_model_takes_the_op_by_op_arithmetic_on_the_cpu():
    import models
    blocks = _tiny_blocks()
    torch.manual_seed(1)
    fused = models.SAGE(6, 8, 3, 2, 0.0, fused=True, aggregator="pool")
    plain = models.SAGE(6, 8, 3, 2, 0.0, fused=False, aggregator="pool")
    split = {}  # the fused layout into the op-by-op model: through split_state_dict, as FusedSAGEConv's
    for i, l in enumerate(fused.layers):
        split.update(l.split_state_dict("layers.%d." % i))
    plain.load_state_dict(split, strict=True)
    fused.load_state_dict(plain.state_dict(), strict=True)
    x = torch.randn(12, 6, generator=torch.Generator().manual_seed(2))
    res = []
    for m in (fused, plain):
        xin = x.clone().requires_grad_()
        y = m(blocks, xin)
        y.square().sum().backward()
        res.append((y.detach(), xin.grad, {k: p.grad for k, p in m.named_parameters()}))
    (yf, gxf, f), (yp, gxp, p) = res
    assert yf.shape == (2, 3) and torch.equal(yf, yp) and torch.equal(gxf, gxp)
    for i, l in enumerate(fused.layers):
        pre, d = "layers.%d." % i, l.in_feats
        assert torch.equal(f[pre + "weight"], torch.cat([p[pre + "fc_self.weight"], p[pre + "fc_neigh.weight"]], 1))
        assert torch.equal(f[pre + "bias"], p[pre + "fc_neigh.bias"])
        assert torch.equal(f[pre + "fc_pool.weight"], p[pre + "fc_pool.weight"])
        assert bool(f[pre + "fc_pool.weight"].abs().sum() > 0) and bool(f[pre + "weight"][:, d:].abs().sum() > 0)


@pytest.mark.parametrize("aggregator", ["pool", "mean"])
@pytest.mark.parametrize("fused", [True, False])
def test_layerwise_inference_equals_the_model_on_full_neighbourhood_blocks(aggregator, fused):
    """a 30-node random CSR with one empty row; every layer's block = the whole CSR"""
    import inference
    import models
    rs = np.random.default_rng(3)
    n = 30
    deg = rs.integers(1, 7, n)
    deg[11] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    indices = rs.integers(0, n, int(indptr[-1])).astype(np.uint32)
    col = torch.from_numpy(np.repeat(np.arange(n), deg).astype(np.int32))
    blocks = [_Block(torch.from_numpy(indices.astype(np.int32)), col, n)] * 2
    torch.manual_seed(4)
    model = models.SAGE(6, 8, 3, 2, 0.5, fused=fused, aggregator=aggregator).eval()
    feat = torch.randn(n, 6, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = model(blocks, feat)
    got = inference.layerwise_inference(model, indptr, indices, feat, batch_rows=7)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-5)
