"""CPU-only: the fused GCN / PinSAGE layers exist at every level -- the four kernels' entry points in the built library,
the header and the binding's export list, the layers and the `fused=` switch in examples/models.py -- and off the GPU
the fused models take the op-by-op arithmetic (same numbers, interchangeable state dicts)."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

NEW = ["fgnn_block_degrees", "fgnn_block_aggregate_scaled", "fgnn_relu_l2norm", "fgnn_relu_l2norm_backward"]


def test_library_header_and_binding_carry_the_four_entry_points():
    from fgnn_hip import lib
    so = ctypes.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fgnn_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert hasattr(so, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in lib.EXPORTS, name


def test_layers_and_fused_switch_exist():
    import models
    assert issubclass(models.FusedGraphConv, torch.nn.Module)
    assert issubclass(models.FusedWeightedSAGEConv, torch.nn.Module)
    for cls in (models.GCN, models.PinSAGE):
        assert inspect.signature(cls.__init__).parameters["fused"].default in (True, False)
    assert isinstance(models.GCN(8, 8, 3, 2, 0.0, fused=True).layers[0], models.FusedGraphConv)
    assert type(models.GCN(8, 8, 3, 2, 0.0, fused=False).layers[0]) is models.GraphConv
    assert isinstance(models.PinSAGE(8, 8, 3, 2, 0.0, fused=True).layers[0], models.FusedWeightedSAGEConv)
    assert type(models.PinSAGE(8, 8, 3, 2, 0.0, fused=False).layers[0]) is models.WeightedSAGEConv
    gcn = models.GCN(8, 8, 3, 2, 0.5)
    assert gcn.dropout_step is None and isinstance(gcn.dropout_seed, int)
    assert models.MODELS["gcn"] is models.GCN and models.MODELS["pinsage"] is models.PinSAGE


class _Block:
    def __init__(self, row, col, ndst, w=None):
        self.row, self.col, self.ndst = row, col, ndst
        self.edata = {"weights": w} if w is not None else {}

    def number_of_dst_nodes(self):
        return self.ndst


def _tiny_blocks():
    """a two-layer chain: 12 -> 5 -> 2 nodes, one destination without an edge in each block"""
    g = torch.Generator().manual_seed(4)
    blocks = []
    for nsrc, ndst, E in ((12, 5, 23), (5, 2, 6)):
        row = torch.randint(0, nsrc, (E,), generator=g, dtype=torch.int32)
        col = torch.sort(torch.randint(0, ndst - 1, (E,), generator=g, dtype=torch.int32))[0]
        w = torch.randint(1, 9, (E,), generator=g, dtype=torch.int32)
        blocks.append(_Block(row, col, ndst, w))
    return blocks


@pytest.mark.parametrize("kind", ["gcn", "pinsage"])
def test_fused_models_fall_back_to_the_op_by_op_arithmetic_on_the_cpu(kind):
    import models
    blocks = _tiny_blocks()
    torch.manual_seed(1)
    fused = models.MODELS[kind](6, 8, 3, 2, 0.0, fused=True)
    plain = models.MODELS[kind](6, 8, 3, 2, 0.0, fused=False)
    # state dicts load both ways, no translation
    assert sorted(fused.state_dict()) == sorted(plain.state_dict())
    plain.load_state_dict(fused.state_dict(), strict=True)
    fused.load_state_dict(plain.state_dict(), strict=True)
    x = torch.randn(12, 6, generator=torch.Generator().manual_seed(2))
    res = []
    for m in (fused, plain):
        xin = x.clone().requires_grad_()
        y = m(blocks, xin)
        y.square().sum().backward()
        res.append((y.detach(), xin.grad, [p.grad for p in m.parameters()]))
    assert res[0][0].shape == (2, 3)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
