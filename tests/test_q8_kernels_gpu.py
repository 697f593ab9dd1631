"""The kernels of the 8-bit feature store (csrc/q8_rows.hip through fgnn_hip.lib / fgnn_hip.nn) against the numpy
references of tests/q8_refs.py: the quantiser byte for byte, the decode bit for bit, the aggregation over sampled blocks
and over CSR rows inside (2 k + 8) 2^-23 of the sum of its terms' magnitudes around the float64 sum over the exactly
decoded rows.  Every bounded test prints its worst error / bound ratio before it asserts."""
import numpy as np
import pytest
import torch

import q8_refs as Q
from test_f16_kernels_gpu import hip, nn  # noqa: F401  (the loaded library and fgnn_hip.nn as fixtures)
from train_refs import assert_within as _within  # prints the worst error / bound ratio, then asserts it is <= 1

pytestmark = pytest.mark.gpu
EINVAL = -1
GUARD = 0xA5


def _i32(a):
    return torch.from_numpy(np.asarray(a).astype(np.uint32).view(np.int32)).cuda()


def _framed_rows(rows, pad=32, left=16):
    """the q8 rows as a column block of a wider uint8 matrix (row stride S + pad, a multiple of 16; 16-byte aligned base)"""
    n, S = rows.shape
    big = torch.full((n, S + pad), GUARD, dtype=torch.uint8)
    big[:, left:left + S] = torch.from_numpy(rows)
    big = big.cuda()
    return big, big[:, left:left + S]


# dims: the format's edge cases, the widest single-load row (240), the narrowest walked in passes (241), and one beyond
# the 1024 columns the quantiser holds in registers
@pytest.mark.parametrize("dim", [1, 15, 16, 17, 128, 256, 241, 600, 1100])
def test_quantiser_and_decode_equal_numpy_and_stay_inside_their_rows(hip, dim):  # noqa: F811
    n, S = 37, Q.row_bytes(dim)
    assert hip.q8_row_bytes(dim) == S
    x = Q.features(n, dim, seed=dim)
    xbig = torch.randn((n, dim + 5))
    xbig[:, 3:3 + dim] = torch.from_numpy(x)
    want = Q.encode(x)
    big, rows = _framed_rows(np.zeros((n, S), dtype=np.uint8))
    big[:] = GUARD
    hip.quantize_rows_q8(xbig.cuda()[:, 3:3 + dim], out=rows)
    got = big.cpu().numpy()
    assert got[:, 16:16 + S].tobytes() == want.tobytes()
    assert (got[:, :16] == GUARD).all() and (got[:, 16 + S:] == GUARD).all()
    # decode: all rows in order, and a list that permutes, repeats and omits rows; out a column block of a wider matrix
    dec = Q.decode_f32(want, dim)
    index = np.random.default_rng(dim).integers(0, n, 29)
    for idx, ref in ((None, dec), (index, dec[index])):
        obig = torch.full((len(ref), dim + 7), 7.5, device="cuda")
        hip.dequantize_rows_q8(rows, dim, index=None if idx is None else _i32(idx), out=obig[:, 2:2 + dim])
        o = obig.cpu().numpy()
        assert o[:, 2:2 + dim].tobytes() == ref.tobytes()
        assert (o[:, :2] == 7.5).all() and (o[:, 2 + dim:] == 7.5).all()
    _within(dec, x.astype(np.float64), Q.roundtrip_bound(want, dim), "round trip, dim %d" % dim)


@pytest.mark.parametrize("num_dst,din,pad", [(1, 4, 0), (77, 128, 32), (130, 600, 16)])
def test_sage_finish_z_q8_decodes_the_left_half_and_scales_the_right(nn, hip, num_dst, din, pad):  # noqa: F811
    rows = Q.encode(Q.features(num_dst + 9, din, seed=din))
    _, h = _framed_rows(rows, pad=pad, left=0)
    g = torch.Generator().manual_seed(din)
    z0 = torch.randn((num_dst, 2 * din + 4), generator=g).cuda()
    deg = torch.randint(0, 5, (num_dst,), generator=g).float().cuda()
    za, zb = z0.clone(), z0.clone()
    ia = nn.sage_finish_z(za, h, deg, num_dst, din)
    ib = nn.sage_finish_z(zb, hip.dequantize_rows_q8(h, din), deg, num_dst, din)
    assert torch.equal(za.view(torch.int32), zb.view(torch.int32)) and torch.equal(ia, ib)
    assert za[:, :din].cpu().numpy().tobytes() == Q.decode_f32(rows[:num_dst], din).tobytes()


# ---- sampled blocks ----------------------------------------------------------------------------------------------------------
NSRC, NDST = 50, 12
# run lengths by edge count: single edges whose destinations change inside one four-edge step, runs that cross a
# group's 16 edges, a wave's 64-edge chunk (edges 60 .. 64 of 65; 57 .. 126, 127 .. 226 and 227 .. 256 of 257)
RUNS = {1: (1,), 3: (1, 2), 64: (5, 1, 1, 1, 1, 20, 35), 65: (60, 5), 257: (3, 1, 1, 1, 1, 50, 70, 100, 30)}
DST_ORDER = (4, 0, 9, 2, 11, 5, 1, 8, 3)  # destinations 6, 7 and 10 never have an edge
MODES = ((0, 0), (1, 1), (0, 2), (2, 0), (2, 1))


def _block_cases():
    cases = []
    for i, dim in enumerate((1, 17, 128, 240, 241, 256, 600)):  # 600: three passes over the codes
        for j, e in enumerate(RUNS):
            c = 5 * i + j
            scaled = c % 2 == 1
            cases.append((e, dim, scaled, MODES[(c // 2) % 5] if scaled else (0, 0), c % 3 != 0, not scaled and c % 4 == 0,
                          c % 3 == 1))
    return cases


@pytest.mark.parametrize("case", _block_cases(), ids=lambda c: "e%d-d%d-%s-%d%d-%s%s%s" % (
    c[0], c[1], "scaled" if c[2] else "ex", c[3][0], c[3][1], "w" if c[4] else "1", "-deg" if c[5] else "",
    "-wide" if c[6] else ""))
def test_block_aggregation_over_q8_rows_stays_inside_its_bound(nn, case):
    e, dim, scaled, (src_mode, dst_mode), weighted, count_deg, wide = case
    rs = np.random.default_rng(1000 * e + dim)
    dst = np.repeat(DST_ORDER[:len(RUNS[e])], RUNS[e])
    src = rs.integers(0, NSRC, e)
    w = (0.05 + 1.4 * rs.random(e)).astype(np.float32) if weighted else None
    src_deg = rs.integers(0, 9, NSRC).astype(np.float32) + np.float32(0.37)
    dst_deg = rs.integers(0, 9, NDST).astype(np.float32)
    rows = Q.encode(Q.features(NSRC, dim, seed=dim))
    _, h = _framed_rows(rows, pad=32 if wide else 0, left=16 if wide else 0)
    ref, bound = Q.aggregate(src, dst, w, rows, dim, NDST, src_deg, src_mode, dst_deg, dst_mode)
    big = torch.full((NDST, dim + 24), 3.25, device="cuda")
    out = big[:, 8:8 + dim]
    out.zero_()
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
    if scaled:
        nn.aggregate_scaled_into(out, h, _i32(src), _i32(dst), t(w), t(src_deg) if src_mode else None, src_mode,
                                 t(dst_deg) if dst_mode else None, dst_mode)
    else:
        deg = torch.full((NDST,), 3.0, device="cuda") if count_deg else None
        nn.aggregate_into(out, h, _i32(src), _i32(dst), t(w), in_degree=deg)
        if count_deg:
            assert np.array_equal(deg.cpu().numpy(), 3.0 + np.bincount(dst, minlength=NDST))
    got = big.cpu().numpy()
    _within(got[:, 8:8 + dim], ref, bound, "block")
    assert (got[:, :8] == 3.25).all() and (got[:, 8 + dim:] == 3.25).all()
    assert not got[[6, 7, 10], 8:8 + dim].any()


# ---- CSR rows ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def graph(nn):
    """80 nodes: rows of 0, 1, 4, 5 and 63 edges, one longer than a piece, the rest up to 20 edges"""
    rs = np.random.default_rng(77)
    lens = rs.integers(0, 21, 80)
    lens[:6] = [0, 1, 4, 5, 63, nn.csr_split_length() + 77]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = rs.integers(0, 80, indptr[-1])
    w = (0.05 + 1.4 * rs.random(indptr[-1])).astype(np.float32)
    src_deg = rs.integers(0, 9, 80).astype(np.float32)
    return indptr, indices, w, src_deg


@pytest.mark.parametrize("dim", [17, 128, 241, 600])
def test_csr_aggregation_over_q8_rows_is_bounded_and_reproducible(nn, graph, dim):
    indptr, indices, w, src_deg = graph
    n = len(indptr) - 1
    rows = Q.encode(Q.features(n, dim, seed=3 * dim))
    _, h = _framed_rows(rows, pad=16, left=0)
    dst = np.repeat(np.arange(n), np.diff(indptr))
    ref, bound = Q.aggregate(indices, dst, w, rows, dim, n, src_deg, 1, np.diff(indptr), 2)
    d_indptr, d_indices, d_w, d_deg = _i32(indptr), _i32(indices), torch.from_numpy(w).cuda(), torch.from_numpy(src_deg).cuda()

    def run(nodes=None, max_edges=None):
        count = n if nodes is None else len(nodes)
        big = torch.full((count, dim + 6), 9.5, device="cuda")
        nn.csr_aggregate_into(big[:, 2:2 + dim], h, d_indptr, d_indices, nodes=None if nodes is None else _i32(nodes),
                              edge_weight=d_w, src_deg=d_deg, src_mode=1, dst_mode=2, max_edges=max_edges)
        got = big.cpu().numpy()
        assert (got[:, :2] == 9.5).all() and (got[:, 2 + dim:] == 9.5).all()
        return np.ascontiguousarray(got[:, 2:2 + dim])

    full = run()
    _within(full, ref, bound, "csr, dim %d" % dim)
    assert not full[0].any()
    assert run().tobytes() == full.tobytes()                 # two calls: the same bits
    assert run(max_edges=10).tobytes() == full.tobytes()     # an understated bound: the owner wave sums the long row
    subset = np.array([5, 0, 4, 33, 2, 79, 1])
    assert run(nodes=subset).tobytes() == full[subset].tobytes()


def test_bad_q8_rows_are_refused_before_any_launch(hip):  # noqa: F811
    L, dim, S = hip.load(), 16, 32
    idx = torch.zeros(8, dtype=torch.int32, device="cuda")
    h = torch.zeros((4, S + 16), dtype=torch.uint8, device="cuda")
    out = torch.zeros((4, dim), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    ex = lambda hp, ld, d=dim: L.fgnn_block_aggregate_ex_q8(p(idx), p(idx), None, 8, hp, ld, d, p(out), dim, None, st)  # noqa: E731
    # a base that is not 16-byte aligned, a stride that is no multiple of 16 or below a row, no rows, no columns
    assert [ex(p(h) + 4, S + 16), ex(p(h), S + 8), ex(p(h), S - 16), ex(None, S), ex(p(h), S, 0)] == [EINVAL] * 5
    assert L.fgnn_dequantize_rows_q8(p(h) + 4, S, None, 4, dim, p(out), dim, st) == EINVAL
    assert L.fgnn_quantize_rows_q8(p(out), dim, 4, dim, p(h), S - 16, st) == EINVAL
    assert L.fgnn_csr_aggregate_q8(p(idx), p(idx), None, None, 0, 4, 8, p(h), S + 8, dim, p(out), dim, None, 0, None, 0,
                                   None, 0, st) == EINVAL
    torch.cuda.synchronize()
    assert not out.any() and ex(p(h), S + 16) == 0
