"""CPU-only: the fused GAT layer exists at every level -- the three entry points in the built library, the header and
the binding's export list, the layers, the model and the `fused=` switch in examples/models.py -- and off the GPU the
fused model takes the op-by-op arithmetic (same numbers, interchangeable state dicts)."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

NEW = {"fgnn_gat_workspace_bytes": "size_t", "fgnn_gat_forward": "int", "fgnn_gat_backward": "int"}


def test_library_header_and_binding_carry_the_three_entry_points():
    from fgnn_hip import lib
    so = ctypes.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "fgnn_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, ret in NEW.items():
        assert hasattr(so, name), name
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), name
        assert name in lib.EXPORTS and name in lib.SIGNATURES, name
    decl = re.search(r"int\s+fgnn_gat_forward\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
    for arg in ("src_index", "dst_index", "num_edge", "el", "er", "feat", "num_dst", "negative_slope", "attn_p", "seed",
                "const unsigned long long *d_step", "tag", "alpha", "out", "out_ld", "ws", "ws_bytes", "stream"):
        assert arg in decl, arg
    decl = re.search(r"int\s+fgnn_gat_backward\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
    for arg in ("alpha", "gout", "gout_ld", "gfeat", "gfeat_ld", "gel", "ger", "d_step", "ws_bytes"):
        assert arg in decl, arg
    # the workspace query needs no GPU
    so.fgnn_gat_workspace_bytes.restype = ctypes.c_size_t
    so.fgnn_gat_workspace_bytes.argtypes = [ctypes.c_size_t] * 3
    assert so.fgnn_gat_workspace_bytes(1000, 10, 8) >= (1000 * 8 + 3 * 10 * 8) * 4
    assert so.fgnn_gat_workspace_bytes(2000, 10, 8) > so.fgnn_gat_workspace_bytes(1000, 10, 8)


def test_the_shipped_library_still_reads_no_switch():
    from fgnn_hip import lib
    assert b"FGNN_" not in open(lib.LIB_PATH, "rb").read()


def test_layers_model_and_fused_switch_exist():
    import models
    assert issubclass(models.FusedGATConv, models.GATConv) and issubclass(models.GATConv, torch.nn.Module)
    assert models.MODELS["gat"] is models.GAT
    fused, plain = models.GAT(16, 32, 5, 3, 0.5, fused=True), models.GAT(16, 32, 5, 3, 0.5, fused=False)
    assert all(isinstance(l, models.FusedGATConv) for l in fused.layers)
    assert all(type(l) is models.GATConv for l in plain.layers)
    assert models.GAT(16, 32, 5, 2, 0.5).fused is True
    assert fused.dropout_step is None and isinstance(fused.dropout_seed, int)
    # 8 heads of 32 // 8 features inside, out_heads of n_classes at the end; attention dropout defaults to dropout
    assert [(l.num_heads, l.out_feats) for l in fused.layers] == [(8, 4), (8, 4), (1, 5)]
    assert all(l.attn_drop.p == 0.5 and l.feat_drop.p == 0.5 for l in fused.layers)
    assert models.GAT(16, 32, 5, 2, 0.5, attn_drop=0.25, heads=4, out_heads=2).layers[1].attn_drop.p == 0.25
    with pytest.raises(AssertionError):
        models.GAT(16, 30, 5, 2, 0.5)  # 30 is no multiple of 8 heads
    # DGL's parameter names and shapes
    sd = models.GATConv(16, 4, 8, residual=True).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "fc.weight": (32, 16), "attn_l": (1, 8, 4), "attn_r": (1, 8, 4), "bias": (32,), "res_fc.weight": (32, 16)}
    assert "res_fc.weight" not in models.GATConv(32, 4, 8, residual=True).state_dict()  # identity residual


class _Block:
    def __init__(self, row, col, ndst):
        self.row, self.col, self.ndst = row, col, ndst
        self.edata = {}

    def number_of_dst_nodes(self):
        return self.ndst


def _tiny_blocks():
    """a two-layer chain: 12 -> 5 -> 2 nodes, one destination without an edge in each block"""
    g = torch.Generator().manual_seed(4)
    blocks = []
    for nsrc, ndst, E in ((12, 5, 23), (5, 2, 6)):
        row = torch.randint(0, nsrc, (E,), generator=g, dtype=torch.int32)
        col = torch.sort(torch.randint(0, ndst - 1, (E,), generator=g, dtype=torch.int32))[0]
        blocks.append(_Block(row, col, ndst))
    return blocks


@pytest.mark.parametrize("residual", [False, True])
def test_fused_gat_falls_back_to_the_op_by_op_arithmetic_on_the_cpu(residual):
    import models
    blocks = _tiny_blocks()
    torch.manual_seed(1)
    fused = models.GAT(6, 8, 3, 2, 0.0, fused=True, heads=2, out_heads=2, residual=residual)
    plain = models.GAT(6, 8, 3, 2, 0.0, fused=False, heads=2, out_heads=2, residual=residual)
    assert sorted(fused.state_dict()) == sorted(plain.state_dict())
    assert ("layers.1.res_fc.weight" in fused.state_dict()) == residual
    plain.load_state_dict(fused.state_dict(), strict=True)
    fused.load_state_dict(plain.state_dict(), strict=True)
    with torch.no_grad():  # (DGL initialises the bias with zeros: give it a value)
        for m in (fused, plain):
            for l in m.layers:
                l.bias.copy_(torch.linspace(-1, 1, l.bias.numel()))
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
    assert all(g is not None and bool(g.abs().sum() > 0) for g in res[0][2])
