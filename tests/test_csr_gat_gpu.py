"""The GAT attention kernel over whole CSR rows (csrc/csr_gat_attention.hip; fgnn_hip.nn.csr_gat_attention_into) on the
synthetic graph of tests/csr_refs.py, whose special rows sit on every boundary of the kernel: the 4-row unroll, the
wave's 64-entry chunks, the split length on both sides, a row of several pieces with a tail, a hub of 100 000
neighbours, empty rows next to the hubs.  Against the float64 reference every output stays within 4 x the deviation of
the torch fp32 formulation on the same inputs + 2^-22 |ref| (tests/csr_gat_refs.py); on top of that the kernel promises
overwrite semantics and bit-reproducible rows, whatever else a call computes.  Every accuracy test prints the deviation
and its worst error / bound ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import csr_gat_refs as G
import csr_refs as R
import gat_refs
from test_csr_aggregate_gpu import _node_lists

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def nn():
    from fgnn_hip import lib, nn
    lib.load()
    assert torch.cuda.is_available()
    return nn


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


class Graph:
    def __init__(self, nn):
        self.split = nn.csr_split_length()
        self.indptr, self.indices = G.graph(self.split)
        self.d_indptr, self.d_indices = _dev(self.indptr), _dev(self.indices)
        self.rows = R.special_rows(self.split)
        self.lengths = np.diff(self.indptr.astype(np.int64))
        self.d_big = _dev(G.feature_matrix())
        self._scores = {}

    def feat(self, H, F):
        """[N, H, F]: a column block of the wide matrix"""
        return self.d_big[:, G.F_OFF:G.F_OFF + H * F].unflatten(1, (H, F))

    def scores(self, H, kind):
        if (H, kind) not in self._scores:
            self._scores[H, kind] = tuple(_dev(t) for t in G.scores(H, kind))
        return self._scores[H, kind]


@pytest.fixture(scope="module")
def g(nn):
    return Graph(nn)


def _nan_out(rows, H, F):
    """(obig, out): a NaN-filled matrix and its column block O_OFF .. O_OFF + H F as [rows, H, F]"""
    obig = torch.full((rows, H * F + G.O_PAD), float("nan"), dtype=torch.float32, device="cuda")
    return obig, obig[:, G.O_OFF:G.O_OFF + H * F].unflatten(1, (H, F))


def _padding_is_untouched_nan(obig, dim):
    pad = torch.cat([obig[:, :G.O_OFF], obig[:, G.O_OFF + dim:]], 1).contiguous().view(torch.int32)
    return bool((pad == torch.tensor(float("nan")).view(torch.int32).item()).all())


def _special_rows_checks(g, got, H, F, kind, order, what):
    """got [R, H, F] on the host, the special rows in `order`"""
    k = g.lengths[g.rows][order]
    assert np.isfinite(got).all()
    assert (got[k == 0] == 0).all() and (k == 0).sum() >= 5
    G.check(got, H, F, kind, g.split, order, what)


# ---- accuracy and overwrite semantics -----------------------------------------------------------------------------------

@pytest.mark.parametrize("hf", gat_refs.HEADS_FEATS, ids=lambda hf: "%dx%d" % hf)
def test_rows_stay_inside_the_bound_and_overwrite(nn, g, hf):
    """the special rows as a range call and as a reversed node list, out a NaN-filled column block and feat a column
    block too: every addressed element finite and inside the bound, empty rows exactly zero, a row of one edge its
    neighbour's feat row bit for bit, the padding columns still the very NaN"""
    H, F = hf
    el, er = g.scores(H, "normal")
    feat = g.feat(H, F)
    first, count = int(g.rows[0]), len(g.rows)
    one = int(np.flatnonzero(g.lengths[g.rows] == 1)[0])
    neighbour = int(g.indices[g.indptr[g.rows[one]]])
    for what, order, kw in (("range", slice(None), dict(first=first, count=count)),
                            ("reversed list", slice(None, None, -1),
                             dict(nodes=_dev(g.rows[::-1].astype(np.uint32))))):
        obig, out = _nan_out(count, H, F)
        nn.csr_gat_attention_into(out, feat, el, er, g.d_indptr, g.d_indices, **kw)
        assert _padding_is_untouched_nan(obig, H * F)
        got = out.cpu().numpy()
        _special_rows_checks(g, got, H, F, "normal", order, what)
        at = one if what == "range" else count - 1 - one
        assert torch.equal(out[at].view(torch.int32), feat[neighbour].view(torch.int32))


@pytest.mark.parametrize("hf", [(8, 32), (3, 7)], ids=lambda hf: "%dx%d" % hf)
def test_scores_that_overflow_without_the_max(nn, g, hf):
    """el, er uniform in +-50: finite and inside the bound on every special row, the 100 000-edge hub and the row of
    3 split + 5 edges (pieces with different maxima, combined by exp(m_k - m)) among them"""
    H, F = hf
    el, er = g.scores(H, "overflow")
    obig, out = _nan_out(len(g.rows), H, F)
    nn.csr_gat_attention_into(out, g.feat(H, F), el, er, g.d_indptr, g.d_indices, first=int(g.rows[0]),
                              count=len(g.rows))
    assert {R.HUB, 3 * g.split + 5} <= set(g.lengths[g.rows].tolist())
    _special_rows_checks(g, out.cpu().numpy(), H, F, "overflow", slice(None), "overflow")


# ---- determinism ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hf", [(8, 32), (4, 33)], ids=lambda hf: "%dx%d" % hf)
def test_rows_are_bitwise_reproducible_whatever_else_the_call_computes(nn, g, hf):
    """[0, N) in one call, twice: bitwise equal.  The same rows through node lists of 7 shuffled ids (one id twice; the
    hub rows among them): bitwise equal to the full call's rows -- with the default max_edges, with the exact one, and,
    for the list that holds the 100 000-neighbour row twice, with bounds that do not hold, so that one or both copies
    are left to their owner waves."""
    H, F = hf
    el, er = g.scores(H, "normal")
    feat = g.feat(H, F)
    (_, full), (_, again) = _nan_out(R.NUM_NODE, H, F), _nan_out(R.NUM_NODE, H, F)
    nn.csr_gat_attention_into(full, feat, el, er, g.d_indptr, g.d_indices)
    nn.csr_gat_attention_into(again, feat, el, er, g.d_indptr, g.d_indices)
    assert torch.equal(full.view(torch.int32), again.view(torch.int32))
    assert bool(torch.isfinite(full).all())
    for j, nodes in enumerate(_node_lists(g)):
        d_nodes = _dev(nodes.astype(np.uint32))
        want = full[torch.from_numpy(nodes).cuda()].view(torch.int32)
        bounds = (None, int(g.lengths[nodes].sum()))
        if j == 0:  # bounds that do not hold: room for one copy of the hub, for no hub, no workspace at all
            bounds += (R.HUB + 2 * g.split, 2 * g.split, g.split)
        for max_edges in bounds:
            _, some = _nan_out(len(nodes), H, F)
            nn.csr_gat_attention_into(some, feat, el, er, g.d_indptr, g.d_indices, nodes=d_nodes, max_edges=max_edges)
            assert torch.equal(some.view(torch.int32), want), (nodes, max_edges)
    # and the full call is right where the reference was computed
    got = full[torch.from_numpy(g.rows).cuda()].cpu().numpy()
    _special_rows_checks(g, got, H, F, "normal", slice(None), "full call")


# ---- arguments ------------------------------------------------------------------------------------------------------------

def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def test_argument_checks(nn, g):
    from fgnn_hip import lib
    L = lib.load()
    H, F = 8, 32
    D = H * F
    first, count, E = int(g.rows[0]), len(g.rows), len(g.indices)
    el, er = g.scores(H, "normal")
    feat = g.feat(H, F)
    max_heads = nn.csr_gat_max_heads()
    assert max_heads >= 16
    nbytes = L.fgnn_csr_gat_workspace_bytes(count, E, H, F)
    assert nbytes > 0 and L.fgnn_csr_gat_workspace_bytes(count, g.split, H, F) == 0
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full((count, D), float("nan"), dtype=torch.float32, device="cuda")
    nan_bits = out.view(torch.int32).clone()

    def call(**over):
        a = dict(indptr=_p(g.d_indptr), indices=_p(g.d_indices), nodes=None, first=first, num_rows=count, max_edges=E,
                 el=_p(el), er=_p(er), feat=_p(feat), feat_ld=feat.stride(0), num_head=H, num_feat=F, slope=G.SLOPE,
                 out=_p(out), out_ld=D, ws=_p(ws), ws_bytes=nbytes, stream=st)
        a.update(over)
        return L.fgnn_csr_gat_attention(*a.values())

    def off(t, nbytes_off):
        return C.c_void_p(t.data_ptr() + nbytes_off)

    bad = [dict(indptr=None), dict(indices=None), dict(el=None), dict(er=None), dict(feat=None), dict(out=None),
           dict(ws=None),
           dict(indptr=off(g.d_indptr, 2)), dict(indices=off(g.d_indices, 1)), dict(nodes=off(g.d_indices, 2)),
           dict(el=off(el, 2)), dict(er=off(er, 1)), dict(feat=off(feat, 2)), dict(out=off(out, 1)), dict(ws=off(ws, 8)),
           dict(num_head=0), dict(num_feat=0), dict(feat_ld=D - 1), dict(out_ld=D - 1),
           dict(num_head=max_heads + 1, num_feat=1),  # more heads than the staging holds
           dict(ws_bytes=nbytes - 1),                 # one byte short
           dict(first=2 ** 32 - 10), dict(max_edges=2 ** 32)]
    for over in bad:
        assert call(**over) == EINVAL, over
    # num_rows == 0: FGNN_OK whatever else is passed, nothing touched
    assert call(num_rows=0) == 0 and call(num_rows=0, feat=None, out=None, ws=None, num_head=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), nan_bits)
    assert call() == 0
    torch.cuda.synchronize()
    _special_rows_checks(g, out.cpu().numpy().reshape(count, H, F), H, F, "normal", slice(None), "raw call")
