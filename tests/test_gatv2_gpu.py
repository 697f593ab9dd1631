"""The GATv2 kernels (csrc/gatv2_attention.hip) on the GPU against the plain torch formulation in float64 on the CPU,
within bounds measured by DESIGN.md 4.5's procedure on each case's own inputs (the same formulation in float32 is the
yardstick); GATv2(fused=True) against GATv2(fused=False); the argument checks.  Block: gat_refs.gat_block (2000 sources,
300 destinations, 9203 edges: a destination without an edge, one with one, one with 200, a hub of 6001).
tests/test_gatv2_host.py imports the reference, the inputs and the bounds from here."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

import gat_refs as gr  # noqa: E402
from fgnn_hip.nn import gatv2_backward_into, gatv2_forward_into, gatv2_workspace  # noqa: E402
from models import GATv2, FusedGATv2Conv  # noqa: E402

NSRC, NDST, SLOPE = gr.NSRC, gr.NDST, gr.SLOPE
QUANTITIES = ("alpha", "out", "gfs", "gfd", "gattn")
# (edge order, H, F, kind): every reduction path of the score kernel (1, 32 and 64 lanes per head; 7 and 33: the
# per-(edge, head) path) and, at 8 x 64, a second trip of 256 columns; inputs uniform in +-50; attention dropout 0.6
CASES = [(o, H, F, "normal") for o in ("gat_sorted", "gat_unsorted")
         for H, F in ((1, 1), (3, 7), (8, 32), (4, 33), (2, 64), (8, 64))]
CASES += [("gat_sorted", 8, 32, "overflow"), ("gat_unsorted", 3, 7, 0.6)]
# beyond the issue's list: a head of 320 columns spans five trips of 64, and with F above the 300 destinations the
# workspace has no room for gattn's double sums (fp32 atomics on gattn itself)
CASES += [("gat_sorted", 1, 320, "normal")]


def gatv2_ref(row, col, fs, fd, attn, out0, gout, ks=None, dtype=torch.float64):
    """GATv2 on a block, op by op in `dtype` on the CPU, gradients by autograd.  ks [E, H]: keep / (1 - q) or None."""
    row, col = torch.as_tensor(row).long(), torch.as_tensor(col).long()
    fs, fd, attn = (torch.as_tensor(t).to(dtype).clone().requires_grad_() for t in (fs, fd, attn))
    s = (torch.nn.functional.leaky_relu(fs[row] + fd[col], SLOPE) * attn).sum(-1)
    m = torch.full((fd.shape[0], fd.shape[1]), float("-inf"), dtype=dtype)
    m = m.scatter_reduce(0, col.unsqueeze(1).expand_as(s), s.detach(), reduce="amax", include_self=True)
    p = torch.exp(s - m[col])
    a = p / torch.zeros_like(m).index_add_(0, col, p)[col]
    at = a if ks is None else a * torch.as_tensor(ks).to(dtype)
    out = torch.as_tensor(out0).to(dtype).index_add(0, col, fs[row] * at.unsqueeze(-1))
    grads = torch.autograd.grad(out, (fs, fd, attn), torch.as_tensor(gout).to(dtype))
    return {k: v.detach().double().numpy() for k, v in zip(QUANTITIES, (a, out) + grads)}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """fp32 numpy arrays, a function of the case only; out0 is zero in the single-edge destination's row"""
    order, H, F, kind = case
    row, col = gr.structure(order)
    rs = np.random.default_rng(1000 * H + 10 * F + CASES.index(case))
    draw = (lambda s: rs.uniform(-50, 50, s)) if kind == "overflow" else rs.standard_normal
    d = dict(row=row, col=col, fs=draw((NSRC, H, F)), fd=draw((NDST, H, F)), attn=rs.standard_normal((H, F)),
             out0=rs.standard_normal((NDST, H, F)), gout=rs.standard_normal((NDST, H, F)))
    d["out0"][gr.DST_ONE] = 0
    d = {k: (v if k in ("row", "col") else v.astype(np.float32)) for k, v in d.items()}
    q = kind if isinstance(kind, float) else 0.0
    ks = gr.keep_scale(gr.philox_keep(gr.DROP_SEED, gr.DROP_STEP, gr.DROP_TAG, row.size, H, q), q) if q else None
    return dict(d, ks=ks, q=q)


@functools.lru_cache(maxsize=None)
def expectation(case):
    """(ref, bound): the float64 run, and 4 x max |float32 run - ref| over the tensor + 2^-22 |ref| per quantity; out
    starts from out0, so (k + 1) 2^-23 (|before| + |after|) joins its bound, k the destination's edge count"""
    d = inputs(case)
    args = [d[k] for k in ("row", "col", "fs", "fd", "attn", "out0", "gout", "ks")]
    ref, t32 = gatv2_ref(*args), gatv2_ref(*args, dtype=torch.float32)
    bound = {q: 4 * np.abs(t32[q] - ref[q]).max() + 2.0 ** -22 * np.abs(ref[q]) for q in QUANTITIES}
    k = np.bincount(d["col"], minlength=NDST)[:, None, None]
    bound["out"] = bound["out"] + (k + 1) * 2.0 ** -23 * (np.abs(d["out0"]) + np.abs(ref["out"]))
    return ref, bound


def check(got, case, what, quantities=QUANTITIES):
    ref, bound = expectation(case)
    return {q: gr.tr.assert_within(got[q], ref[q], bound[q], "%s %s %s" % (what, case, q)) for q in quantities}


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).cuda()


def _run(d, fs, fd, out, gout, gfs, gfd, gattn):
    """forward into `out`, backward into the given accumulators (None: skipped); returns alpha"""
    row, col, attn = _dev(d["row"], torch.int32), _dev(d["col"], torch.int32), _dev(d["attn"])
    key = dict(attn_p=d["q"], seed=gr.DROP_SEED, tag=gr.DROP_TAG,
               d_step=torch.tensor([gr.DROP_STEP, 0], dtype=torch.int64, device="cuda") if d["q"] else None)
    alpha = torch.full((row.numel(), fs.shape[1]), float("nan"), device="cuda")
    gatv2_forward_into(out, alpha, fs, fd, attn, row, col, SLOPE, **key)
    gatv2_backward_into(gfs, gfd, gattn, gout, alpha, fs, fd, attn, row, col, SLOPE, **key)
    torch.cuda.synchronize()
    return alpha


@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward_and_backward_stay_within_the_measured_bounds(hip, case):
    d = inputs(case)
    fs, fd, out, gout = (_dev(d[k]) for k in ("fs", "fd", "out0", "gout"))
    gfs, gfd, gattn = torch.zeros_like(fs), torch.zeros_like(fd), torch.zeros(case[1:3], device="cuda")
    alpha = _run(d, fs, fd, out, gout, gfs, gfd, gattn)
    check({q: t.cpu().numpy() for q, t in zip(QUANTITIES, (alpha, out, gfs, gfd, gattn))}, case, "kernel")
    if not d["q"]:  # a single edge: alpha == 1.0, and its source row arrives in the zero row bit for bit
        e1 = int(np.nonzero(d["col"] == gr.DST_ONE)[0].item())
        assert bool((alpha[e1] == 1.0).all()) and torch.equal(out[gr.DST_ONE], fs[int(d["row"][e1])])
    assert torch.equal(out[gr.DST_NONE], _dev(d["out0"])[gr.DST_NONE])  # no edge: the row stays


def test_column_blocks_of_wider_matrices_and_null_outputs(hip):
    """fs, fd, out, gout and gfs as column blocks (the columns beside them keep every bit); gfd and gattn null"""
    case = ("gat_unsorted", 8, 32, "normal")
    d, (H, F) = inputs(case), case[1:3]
    g = torch.Generator(device="cuda").manual_seed(1)
    big = {k: torch.randn((n, H * F + 13), device="cuda", generator=g)
           for k, n in (("fs", NSRC), ("fd", NDST), ("out0", NDST), ("gout", NDST), ("gfs", NSRC))}
    view = {k: t[:, 5:5 + H * F].unflatten(1, (H, F)) for k, t in big.items()}
    for k in ("fs", "fd", "out0", "gout"):
        view[k].copy_(_dev(d[k]))
    view["gfs"].zero_()
    before = {k: t.clone() for k, t in big.items()}
    alpha = _run(d, view["fs"], view["fd"], view["out0"], view["gout"], view["gfs"], None, None)
    got = dict(alpha=alpha.cpu().numpy(), out=view["out0"].cpu().numpy(), gfs=view["gfs"].cpu().numpy())
    check(got, case, "column blocks", ("alpha", "out", "gfs"))
    for k, t in big.items():
        assert torch.equal(t[:, :5], before[k][:, :5]) and torch.equal(t[:, 5 + H * F:], before[k][:, 5 + H * F:]), k


class Block:
    def __init__(self, row, col, ndst):
        self.row, self.col, self.ndst = row, col, ndst

    def number_of_dst_nodes(self):
        return self.ndst


def test_fused_gatv2_model_matches_the_op_by_op_model(hip):
    """one state dict, dropout 0, a two-block chain (2000 -> 300 -> 60): outputs and every parameter gradient"""
    row, col = gr.structure("fused_sorted")
    g = torch.Generator().manual_seed(31)
    blocks = [Block(_dev(row, torch.int32), _dev(col, torch.int32), NDST),
              Block(torch.randint(0, NDST, (901,), generator=g).int().cuda(),
                    torch.sort(torch.randint(0, 59, (901,), generator=g))[0].int().cuda(), 60)]
    torch.manual_seed(3)
    fused = GATv2(96, 64, 10, 2, 0.0, fused=True, residual=True).cuda()
    plain = GATv2(96, 64, 10, 2, 0.0, fused=False, residual=True).cuda()
    plain.load_state_dict(fused.state_dict(), strict=True)
    assert all(type(l) is FusedGATv2Conv for l in fused.layers)
    gd = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((NSRC, 96), device="cuda", generator=gd)
    gy = torch.randn((60, 10), device="cuda", generator=gd)
    res = []
    for m in (fused, plain):
        y = m(blocks, x)
        y.backward(gy)
        res.append((y.detach(), dict((k, p.grad) for k, p in m.named_parameters())))
    torch.testing.assert_close(res[0][0], res[1][0], rtol=1e-4, atol=1e-4)
    for k, grad in res[0][1].items():
        torch.testing.assert_close(grad, res[1][1][k], rtol=1e-4, atol=1e-4, msg=lambda m, k=k: "%s: %s" % (k, m))


def test_gatv2_entry_points_refuse_bad_arguments_without_a_launch(hip):
    L = hip.load()
    H, F, E = 2, 4, 100
    g = torch.Generator().manual_seed(0)
    row = torch.randint(0, 50, (2 * E,), generator=g).int().cuda()
    col = torch.randint(0, 20, (E,), generator=g).int().cuda()
    fs, fd, attn = torch.ones((50, H, F), device="cuda"), torch.ones((20, H, F), device="cuda"), \
        torch.ones((H, F), device="cuda")
    poison = [torch.full(s, 5.0, device="cuda") for s in ((E, H), (20, H, F), (50, H, F), (20, H, F), (H, F))]
    alpha, out, gfs, gfd, gattn = poison
    ws = gatv2_workspace("cuda", E, 20, H)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def fwd(row_p=p(row), heads=H, ws_bytes=ws.numel() * 4):
        return L.fgnn_gatv2_forward(row_p, p(col), E, p(fs), H * F, p(fd), H * F, p(attn), 20, heads, F, 0.2, 0.0, 1, None,
                                    0, p(alpha), p(out), H * F, p(ws), ws_bytes, st)

    def bwd(row_p=p(row), heads=H, ws_bytes=ws.numel() * 4):
        return L.fgnn_gatv2_backward(row_p, p(col), E, p(fs), H * F, p(fd), H * F, p(attn), p(alpha), p(out), H * F, 20,
                                     heads, F, 0.2, 0.0, 1, None, 0, p(gfs), H * F, p(gfd), H * F, p(gattn), p(ws),
                                     ws_bytes, st)

    with pytest.raises(AssertionError):  # a strided index never reaches the library ...
        gatv2_forward_into(out, alpha, fs, fd, attn, row[::2], col)
    for bad in (dict(row_p=p(row, 2)), dict(ws_bytes=ws.numel() * 4 - 4), dict(heads=0)):  # ... nor a misaligned one
        assert fwd(**bad) == -1 and bwd(**bad) == -1, bad  # FGNN_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == 5.0).all()) for t in poison)  # nothing was launched
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool((alpha != 5.0).all()) and bool((gfs != 5.0).any())
