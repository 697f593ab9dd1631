"""csrc/block_relu_max.hip through fgnn_hip.nn against a numpy loop in float64: out and arg must EQUAL it (a selection);
gx within (k + 8) 2^-23 S of the float64 scatter, S = |what gx held| + the magnitudes of the k terms added (DESIGN.md 4.5:
the start value is part of S).  The fused pool layer against the op-by-op one."""
import os
import sys

import numpy as np
import pytest
import torch
from test_gat_exports import _Block

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSRC, NDST = 200, 40
DIMS = [1, 48, 65, 200, 300]
OFF, PAD, SENTINEL = 3, 7, -7.25  # x / out / gout / gx are columns OFF .. OFF + dim of matrices PAD columns wider


@pytest.fixture(scope="module")
def nn():
    from fgnn_hip import lib, nn
    lib.load()
    assert torch.cuda.is_available()
    return nn


def _edges():
    """seed-major.  Destination 0: no edge; 1: one; 2: edges 1 .. 70 (three wave chunks, two boundaries); 3: rows <= 0
    only; 4: source 7 twice; 5: sources 181 and 180, bit-identical positive rows; 6 also has 181 (two gradient terms)"""
    rs = np.random.default_rng(11)
    per_dst = {1: [9], 2: list(rs.integers(0, 180, 70)), 3: [190, 191, 192, 193, 191], 4: [7, 33, 7],
               5: [12, 181, 40, 180, 181]}
    for v in range(6, NDST):
        per_dst[v] = list(rs.integers(0, 180, rs.integers(3, 13)))
    per_dst[6].append(181)
    row = np.concatenate([per_dst[v] for v in sorted(per_dst)]).astype(np.int32)
    col = np.concatenate([[v] * len(per_dst[v]) for v in sorted(per_dst)]).astype(np.int32)
    assert (col[1:71] == 2).all() and len(row) > 300
    return row, col


def _x(dim):
    x = np.random.default_rng(dim).standard_normal((NSRC, dim)).astype(np.float32)
    x[190] = -0.0
    x[191:194] = -np.abs(x[191:194])
    x[180] = x[181] = np.abs(x[180]) + 10  # the two tied winners of destination 5
    return x


def _reference(row, col, x):
    """edge by edge in float64; a strict > over ascending e keeps the smallest e"""
    m = np.full((NDST, x.shape[1]), -np.inf)
    a = np.full(m.shape, -1, dtype=np.int64)
    for e in range(len(row)):
        better = x[row[e]].astype(np.float64) > m[col[e]]
        m[col[e]][better] = x[row[e]][better]
        a[col[e]][better] = e
    return np.where(m > 0, m, 0.0), np.where(m > 0, a, -1)


@pytest.fixture(scope="module")
def cases():
    row, col = _edges()
    orders = {"sorted": np.arange(len(row)), "shuffled": np.random.default_rng(5).permutation(len(row))}
    return {(dim, o): (row[i], col[i], _x(dim)) + _reference(row[i], col[i], _x(dim))
            for dim in DIMS for o, i in orders.items()}


def _block(a, fill):
    wide = torch.full((a.shape[0], a.shape[1] + PAD), fill, device="cuda")
    wide[:, OFF:OFF + a.shape[1]] = torch.from_numpy(a)
    return wide, wide[:, OFF:OFF + a.shape[1]]


def _intact(wide, dim):
    return bool((wide[:, :OFF] == SENTINEL).all() and (wide[:, OFF + dim:] == SENTINEL).all())


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("dim", DIMS)
def test_forward_equals_the_reference_and_backward_is_within_the_bound(nn, cases, dim, order):
    row, col, x, ref_out, ref_arg = cases[dim, order]
    d_row, d_col = torch.from_numpy(row).cuda(), torch.from_numpy(col).cuda()
    ow, out = _block(np.ones((NDST, dim), np.float32), SENTINEL)
    arg = torch.full((NDST, dim), 12345, dtype=torch.int32, device="cuda")
    nn.block_relu_max_into(out, arg, _block(x, 9.5)[1], d_row, d_col)
    got = out.cpu().numpy()
    assert np.array_equal(got, ref_out.astype(np.float32)) and not np.signbit(got).any() and _intact(ow, dim)
    assert np.array_equal(got, cases[dim, "sorted"][3].astype(np.float32))  # whatever the edge order
    assert np.array_equal(arg.cpu().numpy(), ref_arg)
    assert (ref_arg[0] == -1).all() and (ref_arg[3] == -1).all() and (ref_arg[5] > 0).all()  # the graph is what it says

    rs = np.random.default_rng(dim + 1)
    gout = rs.standard_normal((NDST, dim)).astype(np.float32)
    gx0 = rs.standard_normal((NSRC, dim)).astype(np.float32) + 0.5
    gxw, gx = _block(gx0, SENTINEL)
    nn.block_relu_max_backward_into(gx, arg, d_row, _block(gout, 3.0)[1])
    ref, S, k = gx0.astype(np.float64), np.abs(gx0).astype(np.float64), np.zeros((NSRC, dim))
    v, c = np.nonzero(ref_arg >= 0)
    src = row[ref_arg[v, c]]
    np.add.at(ref, (src, c), gout[v, c].astype(np.float64))
    np.add.at(S, (src, c), np.abs(gout[v, c]).astype(np.float64))
    np.add.at(k, (src, c), 1)
    err, bound = np.abs(gx.cpu().numpy() - ref), (k + 8) * 2.0 ** -23 * S
    print("dim %d %s: worst |gx - ref| / bound = %.3g, most terms in an element %d" % (dim, order, (err / bound).max(),
                                                                                       k.max()))
    assert (err <= bound).all() and k.max() >= 2 and _intact(gxw, dim)
    assert np.array_equal(gx.cpu().numpy()[k == 0], gx0[k == 0])


def test_a_block_without_an_edge_gives_zeros_and_no_winner(nn):
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    ow, out = _block(np.ones((NDST, 65), np.float32), SENTINEL)
    arg = torch.zeros((NDST, 65), dtype=torch.int32, device="cuda")
    nn.block_relu_max_into(out, arg, _block(_x(65), 9.5)[1], none, none)
    assert bool((out == 0).all() and (arg == -1).all()) and _intact(ow, 65)


def test_autograd_node_gives_the_gradient_of_the_into_pair(nn, cases):
    row, col, x, ref_out, _ = cases[65, "shuffled"]
    d_row, d_col = torch.from_numpy(row).cuda(), torch.from_numpy(col).cuda()
    xt = torch.from_numpy(x).cuda().requires_grad_()
    gout = torch.randn((NDST, 65), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    y = nn.block_relu_max(xt, d_row, d_col, NDST)
    y.backward(gout)
    assert np.array_equal(y.detach().cpu().numpy(), ref_out.astype(np.float32))
    arg = torch.empty((NDST, 65), dtype=torch.int32, device="cuda")
    nn.block_relu_max_into(torch.empty_like(y), arg, xt.detach(), d_row, d_col)
    want, S, k = (nn.block_relu_max_backward_into(torch.zeros_like(xt), arg, d_row, g)
                  for g in (gout, gout.abs(), torch.ones_like(gout)))
    # the same terms into zeros in another order: each side is within the bound of the sum
    assert bool(((xt.grad - want).abs() <= 2 * (k + 8) * 2.0 ** -23 * S).all()) and bool(k.max() >= 2)


def _run_layer(layer, blk, x, gy):
    layer.zero_grad()
    h = x.clone().requires_grad_()
    y = layer(blk, h)
    y.backward(gy)
    return y.detach(), h.grad, {k: p.grad.clone() for k, p in layer.named_parameters()}


@pytest.fixture(scope="module")
def layer_case(nn):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import models
    assert models._fused_aggregate is not None
    row, col = _edges()
    blk = _Block(torch.from_numpy(row).cuda(), torch.from_numpy(col).cuda(), NDST)
    torch.manual_seed(6)
    fused, plain = models.FusedSAGEPoolConv(100, 47), models.SAGEConvPool(100, 47)
    plain.load_state_dict(fused.split_state_dict(), strict=True)
    fused, plain = fused.cuda(), plain.cuda()
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn((NSRC, 100), device="cuda", generator=g)
    gy = torch.randn((NDST, 47), device="cuda", generator=g)
    return blk, fused, plain, x, gy, _run_layer(fused, blk, x, gy)


def _close(got, want):
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)


def test_fused_pool_layer_matches_the_op_by_op_layer(layer_case):
    """ONE backward: after an optimiser step a near-tie may flip its winner, a discontinuity and not an error"""
    blk, fused, plain, x, gy, got = layer_case
    want = _run_layer(plain, blk, x, gy)
    _close(got[0], want[0])
    _close(got[1], want[1])
    _close(got[2]["weight"], torch.cat([want[2]["fc_self.weight"], want[2]["fc_neigh.weight"]], 1))
    for k, k_plain in (("bias", "fc_neigh.bias"), ("fc_pool.weight", "fc_pool.weight"), ("fc_pool.bias", "fc_pool.bias")):
        _close(got[2][k], want[2][k_plain])
    assert bool(got[2]["weight"][:, 100:].abs().sum() > 0) and bool(got[2]["fc_pool.weight"].abs().sum() > 0)


def test_fused_pool_layer_captures_into_a_graph(nn, layer_case):
    """no host synchronisation, no allocation of the workspace in the capture; every replay re-zeroes the key table"""
    blk, fused, _, x0, gy, want = layer_case
    nn.block_relu_max_workspace(x0.device, NDST, fused.in_feats)
    fused.zero_grad()
    x = torch.zeros_like(x0).requires_grad_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = fused(blk, x)
        y.backward(gy)
    with torch.no_grad():
        x.copy_(x0)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        _close(y.detach(), want[0])
        _close(x.grad, want[1])
        for k, p in fused.named_parameters():
            _close(p.grad, want[2][k])
