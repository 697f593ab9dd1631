"""CPU-only: the float64 GAT reference of tests/gat_refs.py and the bounds derived from it are sound -- the op-by-op
GATConv of examples/models.py agrees with the reference in float64, the Philox mask helper addresses elements like
train_refs.dropout_ref, and an honest fp32 formulation with another summation order passes every bound the GPU tests
use, on the same inputs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gat_refs as gr  # noqa: E402
import train_refs as tr  # noqa: E402


class _Block:
    def __init__(self, row, col, ndst):
        self.row, self.col, self.ndst = row, col, ndst
        self.edata = {}

    def number_of_dst_nodes(self):
        return self.ndst


def _small_block():
    """40 sources, 9 destinations: destination 0 without an edge, 1 with one, 2 with 200, the rest random; unsorted"""
    rs = np.random.default_rng(5)
    col = np.concatenate([np.full(1, 1), np.full(200, 2), rs.integers(3, 9, 60)])
    row = rs.integers(0, 40, col.size)
    perm = rs.permutation(col.size)
    return row[perm], col[perm], 40, 9


@pytest.mark.parametrize("residual", [False, True])
def test_gatconv_in_float64_agrees_with_the_reference(residual):
    """forward and every gradient within 2^-44 of the tensor's largest magnitude (256 ulp of float64 at that scale: sums
    of up to 200 terms in two different orders)"""
    import models
    row, col, nsrc, ndst = _small_block()
    H, F, din = 3, 5, 15 if residual else 11  # residual: identity (din == H F)
    seen = {}

    class Probe(models.GATConv):
        def project(self, block, h):
            r = super().project(block, h)
            for k, t in zip(("feat", "el", "er"), r[1:]):
                t.retain_grad()
                seen[k] = t
            return r

    torch.manual_seed(0)
    layer = Probe(din, F, H, negative_slope=0.2, residual=residual).double()
    with torch.no_grad():
        layer.bias.copy_(torch.linspace(-1, 1, H * F))
    g = torch.Generator().manual_seed(1)
    x = torch.randn((nsrc, din), generator=g, dtype=torch.float64)
    gout = torch.randn((ndst, H, F), generator=g, dtype=torch.float64)
    blk = _Block(torch.from_numpy(row).int(), torch.from_numpy(col).int(), ndst)
    y = layer(blk, x)
    y.backward(gout)
    feat, el, er = (seen[k].detach().numpy() for k in ("feat", "el", "er"))
    out0 = layer.bias.detach().view(1, H, F).expand(ndst, H, F).numpy().copy()
    if residual:
        out0 = out0 + x[:ndst].view(ndst, H, F).numpy()
    ref = gr.gat_ref(row, col, feat, el, er, ndst, 0.2, out0=out0, gout=gout.numpy())
    # feat.grad is the TOTAL gradient: the attention path (gfeat) plus el's and er's through attn_l / attn_r
    total = ref["gfeat"] + ref["gel"][:, :, None] * layer.attn_l.detach().numpy()
    total[:ndst] += ref["ger"][:, :, None] * layer.attn_r.detach().numpy()
    for name, got, want in (("out", y, ref["out"]), ("gel", seen["el"].grad, ref["gel"]),
                            ("ger", seen["er"].grad, ref["ger"]), ("gfeat", seen["feat"].grad, total)):
        tr.assert_within(got, want, torch.tensor(2.0 ** -44 * np.abs(want).max()), "GATConv float64 " + name)
    # the destination without an edge: bias (+ residual) only; the one with a single edge: attention exactly 1
    assert np.array_equal(y.detach().numpy()[0], out0[0])
    e1 = int(np.nonzero(col == 1)[0][0])
    assert np.array_equal(ref["alpha"][e1], np.ones(H))


def test_reference_alpha_is_a_softmax_and_the_overflow_inputs_need_the_max():
    case = ("gat_sorted", 8, 32, "overflow")
    inp = gr.case_inputs(case)
    ref, _, _ = gr.expectation(case)
    s = inp["el"][inp["row"]] + inp["er"][inp["col"]]
    assert s.max() > 88.8 and s.min() < -88.8  # float32 exp overflows above 88.73
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.where(s > 0, s, np.float32(0.2) * s).astype(np.float32))).any()
    sums = np.zeros((gr.NDST, 8))
    np.add.at(sums, inp["col"], ref["alpha"])
    has = np.bincount(inp["col"], minlength=gr.NDST) > 0
    assert np.abs(sums[has] - 1).max() < 1e-12 and not sums[~has].any()
    assert np.isfinite(ref["alpha"]).all() and (ref["alpha"] >= 0).all()


def test_philox_keep_addresses_elements_like_the_relu_dropout_reference():
    E, H, q = 1001, 3, 0.6  # E H = 3003: no multiple of 4
    keep = gr.philox_keep(gr.DROP_SEED, gr.DROP_STEP, gr.DROP_TAG, E, H, q)
    x = np.ones(3004, dtype=np.float32)
    want = tr.dropout_ref(x, q, gr.DROP_SEED, gr.DROP_STEP, gr.DROP_TAG)[:3003] > 0
    assert np.array_equal(keep.reshape(-1), want)
    assert 0.35 < keep.mean() < 0.45
    assert not np.array_equal(keep, gr.philox_keep(gr.DROP_SEED, gr.DROP_STEP + 1, gr.DROP_TAG, E, H, q))
    ks = gr.keep_scale(keep, q)
    assert set(np.unique(ks)) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(q)))}


@pytest.mark.parametrize("case", gr.cases(), ids=gr.case_id)
def test_an_honest_fp32_formulation_passes_every_bound(case):
    """the bounds are measured on torch's gather / index_add_ formulation; the per-destination loop in float32 (another
    order of the additions, numpy's exp) must pass them too, or they would be fitted to one formulation"""
    inp = gr.case_inputs(case)
    feat, out0, gout = gr.case_views(inp)
    got = gr.gat_ref(inp["row"], inp["col"], feat, inp["el"], inp["er"], gr.NDST, out0=out0, ks=inp["ks"], gout=gout,
                     dtype=np.float32)
    assert all(got[q].dtype == np.float32 for q in gr.QUANTITIES)
    gr.check(got, case, what="fp32 loop")
