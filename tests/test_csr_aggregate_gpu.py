"""The CSR aggregation kernel (csrc/csr_aggregate.hip; fgnn_hip.nn.csr_aggregate_into) on one synthetic graph whose rows
sit on every boundary of the kernel: the 4-row unroll, the wave's 64-entry index loads, the split length on both sides,
a row of several pieces with a tail, a hub of 100 000 neighbours, empty rows next to the hubs (tests/csr_refs.py).
Against the float64 reference every output stays within (k + 8) 2^-23 sum|terms| (k = the row's length: the bound
csrc/block_aggregate.hip documents); on top of that the kernel promises overwrite semantics and bit-reproducible rows,
whatever else a call computes.  Every accuracy test prints its worst error / bound ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import csr_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -1
DIMS = (1, 3, 64, 65, 128, 130, 256, 300)
WIDTH = 304  # columns of the matrices the tests cut h out of


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
        self.indptr, self.indices = R.synthetic_csr(self.split)
        self.d_indptr, self.d_indices = _dev(self.indptr), _dev(self.indices)
        self.rows = R.special_rows(self.split)
        rng = np.random.default_rng(3)
        self.h = rng.standard_normal((R.NUM_NODE, WIDTH)).astype(np.float32)
        self.h16 = self.h.astype(np.float16)
        self.d_h, self.d_h16 = _dev(self.h), _dev(self.h16)
        # fp16 rows with an odd stride behind a base that is offset by one element
        self.odd_ld = WIDTH - 3
        flat = torch.empty(R.NUM_NODE * self.odd_ld + 1, dtype=torch.float16, device="cuda")
        self.d_h16_odd = flat[1:].view(R.NUM_NODE, self.odd_ld)
        self.d_h16_odd.copy_(self.d_h16[:, :self.odd_ld])
        self.w = rng.standard_normal(len(self.indices)).astype(np.float32)
        self.src_deg = rng.uniform(0, 40, size=R.NUM_NODE).astype(np.float32)
        self.dst_deg = rng.uniform(0, 40, size=R.NUM_NODE).astype(np.float32)
        self.d_w, self.d_src_deg, self.d_dst_deg = _dev(self.w), _dev(self.src_deg), _dev(self.dst_deg)
        self.lengths = np.diff(self.indptr.astype(np.int64))


@pytest.fixture(scope="module")
def g(nn):
    return Graph(nn)


def _check(got, ref, S, k, what):
    bound = R.aggregate_bound(S, k)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(err), np.inf, ratio)
    print("%s: worst |got - ref| / bound = %.4g" % (what, ratio.max()))
    assert ratio.max() <= 1.0, "%s: |got - ref| exceeds its bound %.4g-fold" % (what, ratio.max())


def _nan_out(rows, ld):
    return torch.full((rows, ld), float("nan"), dtype=torch.float32, device="cuda")


def _padding_is_untouched_nan(obig, dim):
    pad = obig[:, dim:].contiguous().view(torch.int32)
    return bool((pad == torch.tensor(float("nan")).view(torch.int32).item()).all())


# ---- accuracy and overwrite semantics -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_fp32_rows_stay_inside_the_bound_and_overwrite(nn, g, dim):
    """the special rows as a range call (first, count) into a NaN-filled column block: every addressed element finite
    and inside the bound, empty rows exactly zero, the padding columns still the very NaN"""
    first, count = int(g.rows[0]), len(g.rows)
    ref, S, k = R.csr_aggregate_ref(g.indptr, g.indices, g.h[:, :dim], first=first, count=count)
    obig = _nan_out(count, dim + 5)
    nn.csr_aggregate_into(obig[:, :dim], g.d_h[:, :dim], g.d_indptr, g.d_indices, first=first, count=count)
    got = obig[:, :dim].cpu().numpy()
    assert np.isfinite(got).all()
    assert (got[k == 0] == 0).all() and (k == 0).sum() >= 5
    assert _padding_is_untouched_nan(obig, dim)
    _check(got, ref, S, k, "fp32 dim %d" % dim)


@pytest.mark.parametrize("dim", DIMS)
def test_fp16_rows_are_upcast_exactly(nn, g, dim):
    """half rows out of an even-stride matrix: two columns per lane for even dim, one for odd dim"""
    nodes = g.rows[::-1].copy()
    ref, S, k = R.csr_aggregate_ref(g.indptr, g.indices, g.h16[:, :dim], nodes=nodes)
    obig = _nan_out(len(nodes), dim + 2)
    nn.csr_aggregate_into(obig[:, :dim], g.d_h16[:, :dim], g.d_indptr, g.d_indices, nodes=_dev(nodes.astype(np.uint32)))
    got = obig[:, :dim].cpu().numpy()
    assert np.isfinite(got).all() and (got[k == 0] == 0).all() and _padding_is_untouched_nan(obig, dim)
    _check(got, ref, S, k, "fp16 dim %d" % dim)


@pytest.mark.parametrize("dim", (64, 129, 256))
def test_fp16_rows_with_an_odd_stride_and_an_offset_base(nn, g, dim):
    """h_ld odd and the base one element off a 4-byte boundary: one column per lane, the same sums"""
    h = g.d_h16_odd[:, :dim]
    assert h.stride(0) % 2 == 1 and h.data_ptr() % 4 == 2
    first, count = int(g.rows[0]), len(g.rows)
    ref, S, k = R.csr_aggregate_ref(g.indptr, g.indices, g.h16[:, :dim], first=first, count=count, w=g.w, dst_mode=2)
    out = _nan_out(count, dim)
    nn.csr_aggregate_into(out, h, g.d_indptr, g.d_indices, first=first, count=count, edge_weight=g.d_w, dst_mode=2)
    _check(out.cpu().numpy(), ref, S, k, "fp16 odd stride dim %d" % dim)
    if dim % 2 == 0:  # the paired path over the same values: the same additions in the same order
        paired = _nan_out(count, dim)
        nn.csr_aggregate_into(paired, g.d_h16[:, :dim], g.d_indptr, g.d_indices, first=first, count=count,
                              edge_weight=g.d_w, dst_mode=2)
        assert torch.equal(paired.view(torch.int32), out.view(torch.int32))


# ---- scalings ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dst_mode", [0, 1, 2])
@pytest.mark.parametrize("src_mode", [0, 1, 2])
def test_degree_modes_and_edge_weights(nn, g, src_mode, dst_mode, weighted):
    dim = 65
    nodes = g.rows
    ref, S, k = R.csr_aggregate_ref(g.indptr, g.indices, g.h[:, :dim], nodes=nodes, w=g.w if weighted else None,
                                    src_deg=g.src_deg, src_mode=src_mode, dst_deg=g.dst_deg, dst_mode=dst_mode)
    out = _nan_out(len(nodes), dim)
    nn.csr_aggregate_into(out, g.d_h[:, :dim], g.d_indptr, g.d_indices, nodes=_dev(nodes.astype(np.uint32)),
                          edge_weight=g.d_w if weighted else None, src_deg=g.d_src_deg if src_mode else None,
                          src_mode=src_mode, dst_deg=g.d_dst_deg if dst_mode else None, dst_mode=dst_mode)
    _check(out.cpu().numpy(), ref, S, k, "modes %d / %d %s" % (src_mode, dst_mode, "weighted" if weighted else ""))


@pytest.mark.parametrize("dst_mode", [1, 2])
def test_row_length_default_equals_an_explicit_length_vector_bitwise(nn, g, dst_mode):
    dim = 128
    first, count = int(g.rows[0]), len(g.rows)
    ref, S, k = R.csr_aggregate_ref(g.indptr, g.indices, g.h[:, :dim], first=first, count=count, dst_mode=dst_mode)
    implied, explicit = _nan_out(count, dim), _nan_out(count, dim)
    nn.csr_aggregate_into(implied, g.d_h[:, :dim], g.d_indptr, g.d_indices, first=first, count=count, dst_mode=dst_mode)
    nn.csr_aggregate_into(explicit, g.d_h[:, :dim], g.d_indptr, g.d_indices, first=first, count=count,
                          dst_deg=_dev(g.lengths.astype(np.float32)), dst_mode=dst_mode)
    assert torch.equal(implied.view(torch.int32), explicit.view(torch.int32))
    _check(implied.cpu().numpy(), ref, S, k, "row-length degree, mode %d" % dst_mode)


# ---- determinism ---------------------------------------------------------------------------------------------------------

def _node_lists(g):
    """lists of 7 shuffled ids that cover the special rows (the hubs too) and some ordinary ones; each list names one
    id twice"""
    rng = np.random.default_rng(9)
    hub = R.SPECIAL_AT + R.special_lengths(g.split).index(R.HUB)
    ids = np.concatenate([g.rows[g.rows != hub], rng.integers(0, R.NUM_NODE, size=19), [0, R.NUM_NODE - 1]])
    ids = rng.permutation(ids)
    out = [rng.permutation(np.concatenate([ids[:5], [hub, hub]]))]  # the first list holds the 100 000-neighbour row twice
    for a in range(5, len(ids), 6):
        out.append(rng.permutation(np.concatenate([ids[a:a + 6], ids[a:a + 1]])))
    assert all(len(l) == 7 for l in out) and (out[0] == hub).sum() == 2
    return out


@pytest.mark.parametrize("case", [("f32", 65), ("f32", 256), ("f16", 128), ("f16", 33)], ids=lambda c: "%s-%d" % c)
def test_rows_are_bitwise_reproducible_whatever_else_the_call_computes(nn, g, case):
    """[0, N) in one call, twice: bitwise equal.  The same rows through node lists of 7 shuffled ids (one id twice; the
    hub rows among them): bitwise equal to the full call's rows -- with the default max_edges, with the exact one, and,
    for the list that holds the 100 000-neighbour row twice, with bounds that do not hold, so that one or both copies
    are left to their owner waves."""
    kind, dim = case
    h = (g.d_h if kind == "f32" else g.d_h16)[:, :dim]
    kw = dict(edge_weight=g.d_w, src_deg=g.d_src_deg, src_mode=1, dst_mode=1)
    full, again = _nan_out(R.NUM_NODE, dim), _nan_out(R.NUM_NODE, dim)
    nn.csr_aggregate_into(full, h, g.d_indptr, g.d_indices, **kw)
    nn.csr_aggregate_into(again, h, g.d_indptr, g.d_indices, **kw)
    assert torch.equal(full.view(torch.int32), again.view(torch.int32))
    assert bool(torch.isfinite(full).all())
    for j, nodes in enumerate(_node_lists(g)):
        d_nodes = _dev(nodes.astype(np.uint32))
        want = full[torch.from_numpy(nodes).cuda()].view(torch.int32)
        bounds = (None, int(g.lengths[nodes].sum()))
        if j == 0:  # bounds that do not hold: room for one copy of the hub, for no hub, no workspace at all
            bounds += (R.HUB + 2 * g.split, 2 * g.split, g.split)
        for max_edges in bounds:
            some = _nan_out(len(nodes), dim)
            nn.csr_aggregate_into(some, h, g.d_indptr, g.d_indices, nodes=d_nodes, max_edges=max_edges, **kw)
            assert torch.equal(some.view(torch.int32), want), (nodes, max_edges)
    # and the full call is right where the reference was computed
    href = (g.h if kind == "f32" else g.h16)[:, :dim]
    ref, S, k = R.csr_aggregate_ref(g.indptr, g.indices, href, nodes=g.rows, w=g.w, src_deg=g.src_deg, src_mode=1,
                                    dst_mode=1)
    _check(full[torch.from_numpy(g.rows).cuda()].cpu().numpy(), ref, S, k, "full call %s dim %d" % case)


# ---- arguments ------------------------------------------------------------------------------------------------------------

def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def test_argument_checks(nn, g):
    from fgnn_hip import lib
    L = lib.load()
    dim, count, E = 8, 64, len(g.indices)
    first = int(g.rows[0])
    h = g.d_h[:, :dim]
    nbytes = L.fgnn_csr_aggregate_workspace_bytes(count, E, dim)
    assert nbytes > 0 and L.fgnn_csr_aggregate_workspace_bytes(count, g.split, dim) == 0
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = _nan_out(count, dim)
    nan_bits = out.view(torch.int32).clone()

    def call(fn=L.fgnn_csr_aggregate, **over):
        a = dict(indptr=_p(g.d_indptr), indices=_p(g.d_indices), w=_p(g.d_w), nodes=None, first=first, num_rows=count,
                 max_edges=E, h=_p(h), h_ld=h.stride(0), dim=dim, out=_p(out), out_ld=dim, src_deg=_p(g.d_src_deg),
                 src_mode=1, dst_deg=_p(g.d_dst_deg), dst_mode=1, ws=_p(ws), ws_bytes=nbytes, stream=st)
        a.update(over)
        return fn(*a.values())

    def off(t, nbytes_off):
        return C.c_void_p(t.data_ptr() + nbytes_off)

    bad = [dict(indptr=None), dict(indices=None), dict(h=None), dict(out=None), dict(ws=None),
           dict(indptr=off(g.d_indptr, 2)), dict(indices=off(g.d_indices, 1)), dict(w=off(g.d_w, 2)),
           dict(nodes=off(g.d_indices, 2)), dict(h=off(g.d_h, 2)), dict(out=off(out, 1)),
           dict(src_deg=off(g.d_src_deg, 2)), dict(dst_deg=off(g.d_dst_deg, 3)), dict(ws=off(ws, 8)),
           dict(dim=0), dict(h_ld=dim - 1), dict(out_ld=dim - 1),
           dict(src_mode=3), dict(src_mode=-1), dict(dst_mode=3), dict(dst_mode=-1),
           dict(src_deg=None),                    # a source mode with no way to its degree
           dict(ws_bytes=nbytes - 1),             # one byte short
           dict(first=2 ** 32 - 10), dict(max_edges=2 ** 32)]
    for over in bad:
        assert call(**over) == EINVAL, over
    assert call(L.fgnn_csr_aggregate_f16, h=off(g.d_h16, 1)) == EINVAL  # half rows: 2-byte alignment
    # num_rows == 0: FGNN_OK whatever else is passed, nothing touched
    assert call(num_rows=0) == 0 and call(num_rows=0, h=None, out=None, ws=None, dim=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), nan_bits)
    # dst_mode without a vector is the row length, src_mode 0 needs no vector; the unchanged call works
    assert call(dst_deg=None) == 0 and call(src_deg=None, src_mode=0) == 0 and call() == 0
    torch.cuda.synchronize()
    ref, S, k = R.csr_aggregate_ref(g.indptr, g.indices, g.h[:, :dim], first=first, count=count, w=g.w,
                                    src_deg=g.src_deg, src_mode=1, dst_deg=g.dst_deg, dst_mode=1)
    _check(out.cpu().numpy(), ref, S, k, "raw call")
