"""The GATv2 attention kernel over whole CSR rows (csrc/csr_gatv2_attention.hip; fgnn_hip.nn.csr_gatv2_attention_into) on
the synthetic graph of tests/csr_refs.py, whose special rows sit on every boundary of the kernel (the block of B edges,
the 64-id chunk, the piece, the multi-piece tail, the queue).  Bound: 4 x the deviation of the torch fp32 formulation
from a float64 loop on the same inputs + 2^-22 |ref|, computed on the CPU, never from the kernel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import csr_gat_refs as G
import csr_refs as R
import gat_refs
from test_csr_aggregate_gpu import _node_lists

pytestmark = pytest.mark.gpu
EINVAL = -1
FD_OFF = 1  # fd's column block of the wide matrix starts here, fs's at G.F_OFF
SHAPES = [hf + (False,) for hf in gat_refs.HEADS_FEATS + ((1, 47), (1, 172))] + [(8, 32, True)]


def _inputs(H, F, kind, shared):
    """(fs, fd [N, H, F] views of the wide matrix, attn [H, F]); 'overflow': attn scaled to scores of about +-60 sigma"""
    big = G.feature_matrix()
    fs, fd = (big[:, o:o + H * F].reshape(R.NUM_NODE, H, F) for o in (G.F_OFF, FD_OFF))
    attn = np.random.default_rng(100 * H + F).standard_normal((H, F)).astype(np.float32)
    if kind == "overflow":
        attn *= np.float32(60 / np.sqrt(F))
    return fs, fs if shared else fd, attn


def gatv2_ref(indptr, indices, fs, fd, attn, rows, slope):
    """(out [len(rows), H, F] in float64, the largest |score|): a loop over the rows, head by head"""
    indptr = indptr.astype(np.int64)
    _, H, F = fs.shape
    out, smax = np.zeros((len(rows), H, F)), 0.0
    for i, v in enumerate(rows):
        src = indices[indptr[v]:indptr[v + 1]].astype(np.int64)
        for h in range(H if src.size else 0):
            f = fs[src, h].astype(np.float64)
            x = f + fd[v, h].astype(np.float64)
            s = np.where(x > 0, x, slope * x) @ attn[h].astype(np.float64)
            p = np.exp(s - s.max())
            out[i, h] = (p / p.sum()) @ f
            smax = max(smax, float(np.abs(s).max()))
    return out, smax


def gatv2_torch32(indptr, indices, fs, fd, attn, rows, slope):
    """the plain torch fp32 formulation (GATv2Conv.forward's ops) of the same rows, head by head"""
    row, col, srcs = G.coo_of_rows(indptr, indices, rows)
    row, col, n = torch.from_numpy(row), torch.from_numpy(col), len(rows)
    fs, fd, attn = (torch.from_numpy(np.ascontiguousarray(t)) for t in (fs[srcs], fd[rows], attn))
    out = torch.zeros((n,) + tuple(fs.shape[1:]))
    for h in range(fs.shape[1]):
        fsr = fs[:, h][row]
        e = (torch.nn.functional.leaky_relu(fsr + fd[:, h][col], slope) * attn[h]).sum(-1)
        m = torch.full((n,), float("-inf")).scatter_reduce(0, col, e, reduce="amax", include_self=True)
        p = torch.exp(e - m[col])
        z = torch.zeros(n).index_add_(0, col, p)
        out[:, h] = torch.zeros(n, fs.shape[2]).index_add_(0, col, fsr * (p / z[col]).unsqueeze(-1))
    return out.numpy()


@functools.lru_cache(maxsize=None)
def expectation(H, F, kind, shared, split):
    """(ref, bound, dev, largest |score|) for the special rows in ascending order"""
    indptr, indices = G.graph(split)
    args = (indptr, indices) + _inputs(H, F, kind, shared) + (R.special_rows(split), G.SLOPE)
    ref, smax = gatv2_ref(*args)
    dev = float(np.abs(gatv2_torch32(*args).astype(np.float64) - ref).max())
    return ref, 4 * dev + 2.0 ** -22 * np.abs(ref), dev, smax


@pytest.fixture(scope="module")
def nn():
    from fgnn_hip import lib, nn
    lib.load()
    assert torch.cuda.is_available()
    return nn


class Graph:
    def __init__(self, nn):
        self.split = nn.csr_split_length()
        self.indptr, self.indices = G.graph(self.split)
        self.d_indptr, self.d_indices = (torch.from_numpy(a.view(np.int32)).cuda() for a in (self.indptr, self.indices))
        self.rows = R.special_rows(self.split)
        self.lengths = np.diff(self.indptr.astype(np.int64))
        self.d_big = torch.from_numpy(G.feature_matrix()).cuda()
        B = nn.csr_gatv2_block_edges()
        assert {1, B - 1, B, B + 1, R.HUB, 3 * self.split + 5} <= set(self.lengths[self.rows].tolist())

    def inputs(self, H, F, kind="normal", shared=False):
        fs, fd = (self.d_big[:, o:o + H * F].unflatten(1, (H, F)) for o in (G.F_OFF, FD_OFF))
        return fs, fs if shared else fd, torch.from_numpy(_inputs(H, F, kind, shared)[2]).cuda()

    def check(self, got, H, F, kind, shared, order, what):
        """got [R, H, F] on the host, the special rows in `order`: finite, empty rows zero, inside the bound"""
        ref, bound, dev, _ = expectation(H, F, kind, shared, self.split)
        k = self.lengths[self.rows][order]
        assert np.isfinite(got).all()
        assert (got[k == 0] == 0).all() and (k == 0).sum() >= 5
        what = "%s %dx%d %s%s" % (what, H, F, kind, " fd=fs" if shared else "")
        print("%s: torch fp32 deviation %.3g" % (what, dev))
        gat_refs.tr.assert_within(got, np.ascontiguousarray(ref[order]), np.ascontiguousarray(bound[order]), what)


@pytest.fixture(scope="module")
def g(nn):
    return Graph(nn)


def _nan_out(rows, H, F):
    """(a NaN-filled matrix, its column block O_OFF .. O_OFF + H F as [rows, H, F])"""
    obig = torch.full((rows, H * F + G.O_PAD), float("nan"), dtype=torch.float32, device="cuda")
    return obig, obig[:, G.O_OFF:G.O_OFF + H * F].unflatten(1, (H, F))


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "%dx%d%s" % (c[0], c[1], "-shared" if c[2] else ""))
def test_rows_stay_inside_the_bound_and_overwrite(nn, g, case):
    """range call and reversed node list into a NaN-filled column block"""
    H, F, shared = case
    fs, fd, attn = g.inputs(H, F, shared=shared)
    first, count = int(g.rows[0]), len(g.rows)
    one = int(np.flatnonzero(g.lengths[g.rows] == 1)[0])
    neighbour = int(g.indices[g.indptr[g.rows[one]]])
    nan_bits = torch.tensor(float("nan")).view(torch.int32).item()
    for what, order, kw in (("range", slice(None), dict(first=first, count=count)),
                            ("reversed list", slice(None, None, -1),
                             dict(nodes=torch.from_numpy(g.rows[::-1].astype(np.int32)).cuda()))):
        obig, out = _nan_out(count, H, F)
        nn.csr_gatv2_attention_into(out, fs, fd, attn, g.d_indptr, g.d_indices, negative_slope=G.SLOPE, **kw)
        pad = torch.cat([obig[:, :G.O_OFF], obig[:, G.O_OFF + H * F:]], 1).contiguous().view(torch.int32)
        assert bool((pad == nan_bits).all())
        g.check(out.cpu().numpy(), H, F, "normal", shared, order, what)
        at = one if what == "range" else count - 1 - one
        assert torch.equal(out[at].view(torch.int32), fs[neighbour].view(torch.int32))


@pytest.mark.parametrize("hf", [(8, 32), (3, 7)], ids=lambda hf: "%dx%d" % hf)
def test_scores_that_overflow_without_the_max(nn, g, hf):
    """attn scaled until scores pass +-88: blocks and pieces with different maxima, rescaled by exp(m - m')"""
    H, F = hf
    fs, fd, attn = g.inputs(H, F, "overflow")
    assert expectation(H, F, "overflow", False, g.split)[3] > 88
    _, out = _nan_out(len(g.rows), H, F)
    nn.csr_gatv2_attention_into(out, fs, fd, attn, g.d_indptr, g.d_indices, first=int(g.rows[0]), count=len(g.rows),
                                negative_slope=G.SLOPE)
    g.check(out.cpu().numpy(), H, F, "overflow", False, slice(None), "overflow")


@pytest.mark.parametrize("hf", [(8, 32), (4, 33)], ids=lambda hf: "%dx%d" % hf)
def test_rows_are_bitwise_reproducible_whatever_else_the_call_computes(nn, g, hf):
    """[0, N) twice, then lists of 7 ids with default, exact and understated max_edges: equal bits"""
    H, F = hf
    fs, fd, attn = g.inputs(H, F)
    (_, full), (_, again) = _nan_out(R.NUM_NODE, H, F), _nan_out(R.NUM_NODE, H, F)
    for out in (full, again):
        nn.csr_gatv2_attention_into(out, fs, fd, attn, g.d_indptr, g.d_indices, negative_slope=G.SLOPE)
    assert torch.equal(full.view(torch.int32), again.view(torch.int32))
    assert bool(torch.isfinite(full).all())
    for j, nodes in enumerate(_node_lists(g)):
        d_nodes = torch.from_numpy(nodes.astype(np.int32)).cuda()
        want = full[torch.from_numpy(nodes).cuda()].view(torch.int32)
        bounds = (None, int(g.lengths[nodes].sum()))
        if j == 0:  # bounds that do not hold: room for one copy of the hub, for no hub, no workspace at all
            bounds += (R.HUB + 2 * g.split, 2 * g.split, g.split)
        for max_edges in bounds:
            _, some = _nan_out(len(nodes), H, F)
            nn.csr_gatv2_attention_into(some, fs, fd, attn, g.d_indptr, g.d_indices, nodes=d_nodes,
                                        negative_slope=G.SLOPE, max_edges=max_edges)
            assert torch.equal(some.view(torch.int32), want), (nodes, max_edges)
    g.check(full[torch.from_numpy(g.rows).cuda()].cpu().numpy(), H, F, "normal", False, slice(None), "full call")


def test_argument_checks(nn, g):
    from fgnn_hip import lib
    L = lib.load()
    H, F = 8, 32
    D = H * F
    first, count, E = int(g.rows[0]), len(g.rows), len(g.indices)
    fs, fd, attn = g.inputs(H, F)
    max_feats = nn.csr_gatv2_max_feats()
    assert max_feats >= 256
    nbytes = L.fgnn_csr_gatv2_workspace_bytes(count, E, H, F)
    assert nbytes > 0 and L.fgnn_csr_gatv2_workspace_bytes(count, g.split, H, F) == 0
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    out = torch.full((count, D), float("nan"), dtype=torch.float32, device="cuda")
    nan_bits = out.view(torch.int32).clone()

    def p(t, off=0):
        return C.c_void_p(t.data_ptr() + off)

    def call(**over):
        a = dict(indptr=p(g.d_indptr), indices=p(g.d_indices), nodes=None, first=first, num_rows=count, max_edges=E,
                 fs=p(fs), fs_ld=fs.stride(0), fd=p(fd), fd_ld=fd.stride(0), attn=p(attn), num_head=H, num_feat=F,
                 slope=G.SLOPE, out=p(out), out_ld=D, ws=p(ws), ws_bytes=nbytes,
                 stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        a.update(over)
        return L.fgnn_csr_gatv2_attention(*a.values())

    bad = [dict(indptr=None), dict(indices=None), dict(fs=None), dict(fd=None), dict(attn=None), dict(out=None), dict(ws=None),
           dict(indptr=p(g.d_indptr, 2)), dict(indices=p(g.d_indices, 1)), dict(nodes=p(g.d_indices, 2)),
           dict(fs=p(fs, 2)), dict(fd=p(fd, 1)), dict(attn=p(attn, 2)), dict(out=p(out, 1)), dict(ws=p(ws, 8)),
           dict(num_head=0), dict(num_feat=0), dict(fs_ld=D - 1), dict(fd_ld=D - 1), dict(out_ld=D - 1),
           dict(num_head=1, num_feat=max_feats + 1), dict(ws_bytes=nbytes - 1), dict(first=2 ** 32 - 10),
           dict(max_edges=2 ** 32)]
    for over in bad:
        assert call(**over) == EINVAL, over
    # num_rows == 0: FGNN_OK whatever else is passed, nothing touched
    assert call(num_rows=0) == 0 and call(num_rows=0, fs=None, out=None, ws=None, num_head=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), nan_bits)
    assert call() == 0
    torch.cuda.synchronize()
    g.check(out.cpu().numpy().reshape(count, H, F), H, F, "normal", False, slice(None), "raw call")
