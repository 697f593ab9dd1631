"""The GAT attention kernels (csrc/gat_attention.hip) on the GPU against the float64 reference and the measured bounds of
tests/gat_refs.py; FusedGATConv / GAT(fused=True) of examples/models.py against their op-by-op counterparts; the
capture contract.  Blocks: 2000 sources, 300 destinations, at most 9203 edges (gat_refs.gat_block: a destination
without an edge, one with a single edge, one with 200, a hub with 6001), sorted and unsorted."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gat_refs as gr  # noqa: E402

NSRC, NDST = gr.NSRC, gr.NDST


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
    def __init__(self, row, col, ndst):
        self.row, self.col, self.ndst = row, col, ndst
        self.edata = {}

    def number_of_dst_nodes(self):
        return self.ndst


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).cuda()


def _device_case(case):
    """the case's inputs on the GPU: feat, out and gout are column blocks of wider matrices"""
    inp = gr.case_inputs(case)
    H, F = inp["H"], inp["F"]
    D = H * F
    d = dict(inp=inp, H=H, F=F, row=_dev(inp["row"], torch.int32), col=_dev(inp["col"], torch.int32),
             el=_dev(inp["el"]), er=_dev(inp["er"]), featbig=_dev(inp["featbig"]), obig=_dev(inp["obig"]),
             gbig=_dev(inp["gbig"]))
    d["feat"] = d["featbig"][:, gr.F_OFF:gr.F_OFF + D].unflatten(1, (H, F))
    d["out"] = d["obig"][:, gr.O_OFF:gr.O_OFF + D].unflatten(1, (H, F))
    d["gout"] = d["gbig"][:, gr.O_OFF:gr.O_OFF + D].unflatten(1, (H, F))
    d["key"] = dict(attn_p=inp["q"], seed=gr.DROP_SEED, tag=gr.DROP_TAG,
                    d_step=torch.tensor([gr.DROP_STEP, 0], dtype=torch.int64, device="cuda") if inp["q"] else None)
    return d


def _forward(d):
    from fgnn_hip.nn import gat_forward_into
    alpha = torch.full((d["row"].numel(), d["H"]), float("nan"), device="cuda")
    before = d["obig"].clone()
    gat_forward_into(d["out"], alpha, d["feat"], d["el"], d["er"], d["row"], d["col"], gr.SLOPE, **d["key"])
    D = d["H"] * d["F"]
    # what lies beside the output block does not change by a bit
    assert torch.equal(d["obig"][:, :gr.O_OFF], before[:, :gr.O_OFF])
    assert torch.equal(d["obig"][:, gr.O_OFF + D:], before[:, gr.O_OFF + D:])
    return alpha, before


def _backward(d, alpha, skip=None, random_init=False):
    """the backward call into accumulators that enter as zeros (the kernel's own result, no further rounding) or, with
    random_init -- and always for the skipped one, which must stay as it is -- with random contents"""
    from fgnn_hip.nn import gat_backward_into
    g = torch.Generator(device="cuda").manual_seed(3)
    acc = dict(gfeat=torch.randn((NSRC, d["H"] * d["F"] + 6), device="cuda", generator=g),
               gel=torch.randn((NSRC, d["H"]), device="cuda", generator=g),
               ger=torch.randn((NDST, d["H"]), device="cuda", generator=g))
    if not random_init:
        for k in acc:
            if k != skip:
                acc[k].zero_()
        acc["gfeat"][:, :2] = 1.5  # what lies beside the column block
        acc["gfeat"][:, 2 + d["H"] * d["F"]:] = -2.5
    start = {k: v.clone() for k, v in acc.items()}
    views = dict(acc, gfeat=acc["gfeat"][:, 2:2 + d["H"] * d["F"]].unflatten(1, (d["H"], d["F"])))
    args = {k: (None if k == skip else v) for k, v in views.items()}
    gat_backward_into(args["gfeat"], args["gel"], args["ger"], d["gout"], alpha, d["feat"], d["el"], d["er"], d["row"],
                      d["col"], gr.SLOPE, **d["key"])
    torch.cuda.synchronize()
    got = {k: (acc[k].double() - start[k].double()).cpu().numpy() for k in acc}
    got["gfeat"] = got["gfeat"][:, 2:2 + d["H"] * d["F"]].reshape(NSRC, d["H"], d["F"])
    return got, acc, start


@pytest.mark.parametrize("case", gr.cases(), ids=gr.case_id)
def test_forward_and_backward_stay_within_the_measured_bounds(hip, case):
    """alpha, out, gfeat, gel, ger against gat_ref.  out enters with random contents (the reference and the torch fp32
    formulation the bound is measured on add to the same contents); the gradient accumulators enter as zeros, so what
    they hold afterwards is the kernels' result with no further rounding"""
    d = _device_case(case)
    alpha, _ = _forward(d)
    torch.cuda.synchronize()
    H, F = d["H"], d["F"]
    out = d["out"].cpu().numpy()
    a = alpha.cpu().numpy()
    assert np.isfinite(a).all() and (a >= 0).all()
    gr.check(dict(alpha=a, out=out), case, ("alpha", "out"), "kernel")
    # the softmax sums to 1 per (destination, head) within k 2^-23
    col = d["inp"]["col"]
    k = np.bincount(col, minlength=NDST)
    sums = np.zeros((NDST, H))
    np.add.at(sums, col, a.astype(np.float64))
    assert (np.abs(sums[k > 0] - 1) <= (k[k > 0, None] + 2) * 2.0 ** -23).all()
    got, acc, start = _backward(d, alpha)
    ref, bound, dev = gr.expectation(case)
    for q in ("gfeat", "gel", "ger"):
        print("kernel %s %s: torch fp32 deviation %.3g" % (gr.case_id(case), q, dev[q]))
        gr.tr.assert_within(got[q], ref[q], bound[q], "kernel %s %s" % (gr.case_id(case), q))
    assert torch.equal(acc["gfeat"][:, :2], start["gfeat"][:, :2]) and torch.equal(acc["gfeat"][:, 2 + H * F:],
                                                                                  start["gfeat"][:, 2 + H * F:])


@pytest.mark.parametrize("H,F", gr.HEADS_FEATS)
@pytest.mark.parametrize("order", ["gat_sorted", "gat_unsorted"])
def test_single_edge_and_edgeless_destinations_are_exact(hip, H, F, order):
    """a destination with one edge: alpha == 1.0 and, from a zero row, out == the source row bit for bit; a destination
    without an edge keeps its pre-filled row bit for bit"""
    d = _device_case((order, H, F, "normal"))
    D = H * F
    d["obig"][gr.DST_ONE, gr.O_OFF:gr.O_OFF + D] = 0
    alpha, before = _forward(d)
    torch.cuda.synchronize()
    col = d["inp"]["col"]
    e1 = int(np.nonzero(col == gr.DST_ONE)[0][0])
    assert (col == gr.DST_ONE).sum() == 1 and (col == gr.DST_NONE).sum() == 0
    assert bool((alpha[e1] == 1.0).all())
    assert torch.equal(d["out"][gr.DST_ONE], d["feat"][int(d["inp"]["row"][e1])])
    assert torch.equal(d["obig"][gr.DST_NONE], before[gr.DST_NONE])
    edgeless = torch.from_numpy(np.bincount(col, minlength=NDST) == 0).cuda()
    assert int(edgeless.sum()) >= 1 and torch.equal(d["obig"][edgeless], before[edgeless])


@pytest.mark.parametrize("skip", ["gfeat", "gel", "ger"])
@pytest.mark.parametrize("case", [("gat_unsorted", 3, 7, 0.6), ("gat_sorted", 8, 32, "normal")], ids=gr.case_id)
def test_backward_skips_a_null_output(hip, case, skip):
    """each output NULL in turn: the other two stay within their bounds, the skipped accumulator is not touched"""
    d = _device_case(case)
    alpha, _ = _forward(d)
    got, acc, start = _backward(d, alpha, skip=skip)
    ref, bound, _ = gr.expectation(case)
    assert torch.equal(acc[skip], start[skip])
    for q in ("gfeat", "gel", "ger"):
        if q != skip:
            gr.tr.assert_within(got[q], ref[q], bound[q], "skip %s: %s" % (skip, q))


def test_backward_adds_to_what_its_outputs_hold(hip):
    """accumulators with random contents on a block whose nodes have a handful of edges (33 edges, 300 destinations):
    after - before against the reference; every one of the k_i atomic additions into element i rounds at the
    accumulator's magnitude, so (k_i + 1) 2^-23 (|before| + |after|) joins the bound (the rounding model of
    train_refs.aggregate_bound; k_i = the edges of the element's node)"""
    case = ("e33", 8, 32, "normal")
    d = _device_case(case)
    alpha, _ = _forward(d)
    got, acc, start = _backward(d, alpha, random_init=True)
    ref, bound, _ = gr.expectation(case)
    H, F = d["H"], d["F"]
    k_src = np.bincount(d["inp"]["row"], minlength=NSRC).astype(np.float64)
    k_dst = np.bincount(d["inp"]["col"], minlength=NDST).astype(np.float64)
    for q, k in (("gfeat", k_src[:, None, None]), ("gel", k_src[:, None]), ("ger", k_dst[:, None])):
        s, e = start[q], acc[q]
        if q == "gfeat":
            s, e = (t[:, 2:2 + H * F].reshape(NSRC, H, F) for t in (s, e))
        slack = (k + 1) * 2.0 ** -23 * (s.abs() + e.abs()).double().cpu().numpy()
        gr.tr.assert_within(got[q], ref[q], bound[q] + slack, "accumulate %s" % q)
        untouched = torch.from_numpy((k == 0).reshape(-1)).cuda()
        assert torch.equal(acc[q][untouched], start[q][untouched])


def test_an_empty_block_touches_nothing(hip):
    from fgnn_hip.nn import gat_forward_into, gat_backward_into
    e = torch.empty(0, dtype=torch.int32, device="cuda")
    feat = torch.ones((5, 2, 3), device="cuda")
    el, er = torch.ones((5, 2), device="cuda"), torch.ones((4, 2), device="cuda")
    out = torch.full((4, 2, 3), 7.0, device="cuda")
    alpha = torch.empty((0, 2), device="cuda")
    gat_forward_into(out, alpha, feat, el, er, e, e)
    gf, gl, gr_ = torch.full((5, 2, 3), 3.0, device="cuda"), torch.full((5, 2), 3.0, device="cuda"), \
        torch.full((4, 2), 3.0, device="cuda")
    gat_backward_into(gf, gl, gr_, out, alpha, feat, el, er, e, e)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((gf == 3.0).all()) and bool((gl == 3.0).all()) and bool((gr_ == 3.0).all())
    L = hip.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.fgnn_gat_forward(None, None, 0, None, None, None, 0, 0, 0, 0, 0.2, 0.0, 0, None, 0, None, None, 0, None, 0,
                              st) == 0


# ---- dropout ---------------------------------------------------------------------------------------------------------------

def _unique_source_block(H, E=1001):
    """E edges from E DIFFERENT sources to 37 destinations, unsorted: gfeat[row[e]] = a~[e] * gout[col[e]] has a single
    term, so with gout == 1 the backward pass shows a~ itself"""
    rs = np.random.default_rng(77)
    row = rs.permutation(NSRC)[:E]
    col = rs.integers(0, 37, E)
    return row, col, rs.standard_normal((NSRC, H)).astype(np.float32), rs.standard_normal((37, H)).astype(np.float32)


@pytest.mark.parametrize("q", [0.6, 0.1])
def test_dropout_mask_is_the_numpy_philox_and_scales_exactly(hip, q):
    """a~ / a is exactly 0 or 1 / (1 - q) -- a~ == fp32(a * fp32(1 / (1 - q))) or +0 -- wherever a > 0, with the keep pattern of
    train_refs' Philox at element e H + h (E H = 3003: no multiple of 4); the forward pass used the same a~ (out == the
    fp32 sum of a~ at F = 1 with feat == 1 within the aggregation bound); an advanced d_step gives another mask"""
    from fgnn_hip.nn import gat_forward_into, gat_backward_into
    H, E = 3, 1001
    row, col, el, er = _unique_source_block(H, E)
    row_d, col_d = _dev(row, torch.int32), _dev(col, torch.int32)
    el_d, er_d = _dev(el), _dev(er)
    feat = torch.ones((NSRC, H, 1), device="cuda")
    step = torch.tensor([gr.DROP_STEP, 0], dtype=torch.int64, device="cuda")
    key = dict(attn_p=q, seed=gr.DROP_SEED, d_step=step, tag=gr.DROP_TAG)
    masks = []
    for trial in range(2):
        out = torch.zeros((37, H, 1), device="cuda")
        alpha = torch.empty((E, H), device="cuda")
        gat_forward_into(out, alpha, feat, el_d, er_d, row_d, col_d, gr.SLOPE, **key)
        gfeat = torch.zeros((NSRC, H, 1), device="cuda")
        gat_backward_into(gfeat, None, None, torch.ones((37, H, 1), device="cuda"), alpha, feat, el_d, er_d, row_d, col_d,
                          gr.SLOPE, **key)
        torch.cuda.synchronize()
        a = alpha.cpu().numpy()
        at = gfeat.cpu().numpy()[row, :, 0]  # a~[e, h]
        assert (a > 0).all()
        keep = gr.philox_keep(gr.DROP_SEED, gr.DROP_STEP + trial, gr.DROP_TAG, E, H, q)
        assert np.array_equal(at != 0, keep)
        assert np.array_equal(at, np.where(keep, a * gr.tr.dropout_scale(q), np.float32(0)).astype(np.float32))
        # forward: out[v, h] = sum of a~ over v's edges
        want = np.zeros((37, H))
        np.add.at(want, col, at.astype(np.float64))
        k = np.bincount(col, minlength=37)[:, None]
        assert (np.abs(out.cpu().numpy()[:, :, 0] - want) <= (k + 8) * 2.0 ** -23 * want).all()
        masks.append(keep)
        step[0] += 1  # what fgnn_adam_step does once per training step
    assert not np.array_equal(masks[0], masks[1])
    assert abs(masks[0].mean() - (1 - q)) < 0.05


# ---- argument checks ----------------------------------------------------------------------------------------------------------

def test_gat_entry_points_refuse_bad_arguments_without_a_launch(hip):
    from fgnn_hip.nn import gat_workspace
    L = hip.load()
    H, F, E = 2, 4, 100
    g = torch.Generator().manual_seed(0)
    row = torch.randint(0, 50, (E,), generator=g).int().cuda()
    col = torch.randint(0, 20, (E,), generator=g).int().cuda()
    feat = torch.ones((50, H * F), device="cuda")
    el, er = torch.ones((50, H), device="cuda"), torch.ones((20, H), device="cuda")
    out = torch.full((20, H * F), 5.0, device="cuda")      # poisoned: must stay as it is
    alpha = torch.full((E, H), -3.0, device="cuda")
    gfeat = torch.full((50, H * F), 5.0, device="cuda")
    gel, ger = torch.full((50, H), 5.0, device="cuda"), torch.full((20, H), 5.0, device="cuda")
    ws = gat_workspace("cuda", E, 20, H)
    assert ws.numel() * 4 >= L.fgnn_gat_workspace_bytes(E, 20, H)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None  # noqa: E731

    def fwd(row_p=p(row), el_p=p(el), feat_p=p(feat), feat_ld=H * F, heads=H, feats=F, attn_p=0.0, alpha_p=p(alpha),
            out_p=p(out), out_ld=H * F, ws_p=p(ws), ws_bytes=ws.numel() * 4):
        return L.fgnn_gat_forward(row_p, p(col), E, el_p, p(er), feat_p, feat_ld, 20, heads, feats, 0.2, attn_p, 1, None, 0,
                                  alpha_p, out_p, out_ld, ws_p, ws_bytes, st)

    def bwd(gout_p=p(out), gout_ld=H * F, gfeat_p=p(gfeat), gfeat_ld=H * F, gel_p=p(gel), alpha_p=p(alpha), heads=H,
            attn_p=0.0, ws_bytes=ws.numel() * 4):
        return L.fgnn_gat_backward(p(row), p(col), E, p(el), p(er), p(feat), H * F, alpha_p, gout_p, gout_ld, 20, heads, F,
                                   0.2, attn_p, 1, None, 0, gfeat_p, gfeat_ld, gel_p, p(ger), p(ws), ws_bytes, st)

    bad_fwd = (dict(row_p=None), dict(el_p=None), dict(feat_p=None), dict(alpha_p=None), dict(out_p=None), dict(ws_p=None),
               dict(heads=0), dict(feats=0), dict(feat_ld=H * F - 1), dict(out_ld=H * F - 1), dict(out_p=p(out, 2)),
               dict(feat_p=p(feat, 2)), dict(row_p=p(row, 1)), dict(attn_p=1.0), dict(attn_p=-0.1),
               dict(attn_p=float("nan")), dict(ws_bytes=ws.numel() * 4 - 4), dict(ws_bytes=0))
    for bad in bad_fwd:
        code = fwd(**bad)
        assert code == -1, (bad, code)  # FGNN_EINVAL
        with pytest.raises(hip.FgnnError):
            hip._check(code, "fgnn_gat_forward")
    bad_bwd = (dict(gout_p=None), dict(alpha_p=None), dict(gout_ld=H * F - 1), dict(gfeat_ld=H * F - 1),
               dict(gfeat_p=p(gfeat, 2)), dict(gel_p=p(gel, 2)), dict(heads=0), dict(attn_p=1.0), dict(ws_bytes=8))
    for bad in bad_bwd:
        assert bwd(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((alpha == -3.0).all())  # nothing was launched
    assert bool((gfeat == 5.0).all()) and bool((gel == 5.0).all()) and bool((ger == 5.0).all())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool((alpha >= 0).all()) and bool((out != 5.0).any()) and bool((gfeat != 5.0).any())


# ---- autograd binding, layers, model -------------------------------------------------------------------------------------------

def test_gat_attention_autograd_matches_the_reference_and_fills_out(hip):
    """the public binding: gradients of feat, el, er and of the pre-filled `out`, whose contents the sums are added to"""
    from fgnn_hip.nn import gat_attention
    case = ("gat_unsorted", 3, 7, "normal")
    inp = gr.case_inputs(case)
    featn, out0, goutn = gr.case_views(inp)
    ref, bound, _ = gr.expectation(case)
    feat, el, er, pre = (_dev(t).requires_grad_() for t in (featn, inp["el"], inp["er"], out0))
    row, col = _dev(inp["row"], torch.int32), _dev(inp["col"], torch.int32)
    y = gat_attention(feat, el, er, row, col, NDST, gr.SLOPE, out=pre * 1.0)
    gout = _dev(goutn)
    y.backward(gout)
    got = dict(out=y.detach().cpu().numpy(), gfeat=feat.grad.cpu().numpy(), gel=el.grad.cpu().numpy(),
               ger=er.grad.cpu().numpy())
    gr.check(got, case, ("out", "gfeat", "gel", "ger"), "autograd")
    assert torch.equal(pre.grad, gout)
    y2 = gat_attention(feat.detach(), el.detach(), er.detach(), row, col, NDST, gr.SLOPE)  # no out: from zeros
    got2 = y2.cpu().numpy().astype(np.float64) + out0
    gr.tr.assert_within(got2, ref["out"], bound["out"] + 2.0 ** -23 * np.abs(ref["out"]), "autograd out from zeros")


def _layer_pair(models, din, H, F, residual):
    torch.manual_seed(din)
    fused = models.FusedGATConv(din, F, H, 0.0, 0.0, 0.2, residual, torch.nn.functional.elu)
    plain = models.GATConv(din, F, H, 0.0, 0.0, 0.2, residual, torch.nn.functional.elu)
    with torch.no_grad():
        fused.bias.copy_(torch.linspace(-1, 1, H * F))
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
    """the tolerances of tests/test_fused_gnn_gpu.py for fused-against-op-by-op pairs"""
    torch.testing.assert_close(got[0], want[0], rtol=1e-4, atol=1e-4)
    if need_gh:
        torch.testing.assert_close(got[1], want[1], rtol=1e-3, atol=1e-4)
    assert sorted(got[2]) == sorted(want[2])
    for k in got[2]:
        torch.testing.assert_close(got[2][k], want[2][k], rtol=1e-4, atol=2e-3)


def _edges(name):
    row, col = gr.structure(name)
    return _dev(row, torch.int32), _dev(col, torch.int32)


@pytest.mark.parametrize("din,H,F", [(96, 8, 8), (100, 3, 7)])
@pytest.mark.parametrize("need_gh", [True, False])
@pytest.mark.parametrize("residual", [False, True])
def test_fused_gat_layer_matches_the_op_by_op_layer(hip, models, din, H, F, need_gh, residual):
    row, col = _edges("fused_sorted")
    blk = Block(row, col, NDST)
    fused, plain = _layer_pair(models, din, H, F, residual)
    assert (fused.res_fc is not None) == residual
    g = torch.Generator(device="cuda").manual_seed(F)
    x = torch.randn((NSRC, din), device="cuda", generator=g)
    gy = torch.randn((NDST, H, F), device="cuda", generator=g)
    got = _run_layer(fused, blk, x, gy, need_gh)
    _check_layer(got, _run_layer(plain, blk, x, gy, need_gh), need_gh)


def test_fused_gat_layer_forward_and_backward_capture_into_a_graph(hip, models):
    """nothing in the layer's forward + backward synchronises with the host, and the replay computes what the eager pass
    computes (attention dropout 0.5 keyed by a device-side step count: the same count, the same mask)"""
    row, col = _edges("fused_sorted")
    blk = Block(row, col, NDST)
    fused, _ = _layer_pair(models, 96, 8, 8, False)
    fused.attn_drop.p = 0.5
    fused.train()
    step = torch.tensor([5, 0], dtype=torch.int64, device="cuda")
    fused.dropout_key = (99, step, 1)
    g = torch.Generator(device="cuda").manual_seed(8)
    x0 = torch.randn((NSRC, 96), device="cuda", generator=g)
    gy = torch.randn((NDST, 8, 8), device="cuda", generator=g)
    want = _run_layer(fused, blk, x0, gy, True)  # eager warm-up: lazy initialisation and the workspace happen here
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


def test_fused_gat_model_trains_like_the_op_by_op_model(hip, models):
    """three Adam steps (fgnn_hip.nn.Adam, its step count set as dropout_step; dropout 0) on a three-block chain from the
    same weights: the losses track each other within rtol 1e-4 / atol 1e-5"""
    from fgnn_hip.nn import Adam
    row, col = _edges("fused_sorted")
    g = torch.Generator().manual_seed(31)
    blocks = [Block(row, col, NDST)]
    for nsrc, ndst, ne in ((NDST, 60, 901), (60, 12, 100)):
        r = torch.randint(0, nsrc, (ne,), generator=g).int().cuda()
        c = torch.sort(torch.randint(0, ndst - 1, (ne,), generator=g))[0].int().cuda()
        blocks.append(Block(r, c, ndst))
    torch.manual_seed(3)
    fused = models.GAT(96, 64, 10, 3, 0.0, fused=True).cuda()
    plain = models.GAT(96, 64, 10, 3, 0.0, fused=False).cuda()
    plain.load_state_dict(fused.state_dict(), strict=True)
    gd = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((NSRC, 96), device="cuda", generator=gd)
    label = torch.randint(0, 10, (12,), device="cuda", generator=gd)
    losses = {}
    for m in (fused, plain):
        opt = Adam(m.parameters(), lr=0.003)
        m.dropout_step = opt.step_count
        m.train()
        losses[m] = []
        for _ in range(3):
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(m(blocks, x), label)
            loss.backward()
            opt.step()
            losses[m].append(loss.detach())
    lf, lp = torch.stack(losses[fused]), torch.stack(losses[plain])
    print("losses fused %s op-by-op %s" % (lf.tolist(), lp.tolist()))
    torch.testing.assert_close(lf, lp, rtol=1e-4, atol=1e-5)
