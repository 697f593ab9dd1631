"""fp16 rows into the fp32 aggregation kernels (fgnn_block_aggregate_ex_f16, fgnn_block_aggregate_scaled_f16,
fgnn_sage_finish_z_f16; fgnn_hip/nn.py dispatches on h.dtype) against the float64 reference of tests/f16_refs.py
evaluated on the upcast values, inside train_refs.aggregate_bound = (k + 8) 2^-23 S with no atol -- the bound of the
fp32 kernels, which holds unchanged because the upcast is exact and the sums are fp32.  On single-flush blocks the
result equals the fp32 entry point fed h.float() bit for bit.  Every test prints the worst error / bound ratio before
it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import f16_refs as F
import train_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


@pytest.fixture(scope="module")
def nn(hip):
    from fgnn_hip import nn
    return nn


def _np(t):
    return None if t is None else t.numpy()


def _check_block(obig, before, out, ref, S, k, dim, what):
    R.assert_within(out, torch.from_numpy(ref), F.bound(S, k), what)
    assert torch.equal(obig[:, :R.O_OFF], before[:, :R.O_OFF])
    assert torch.equal(obig[:, R.O_OFF + dim:], before[:, R.O_OFF + dim:])
    untouched = torch.from_numpy(k == 0).cuda()
    assert torch.equal(out[untouched], before[:, R.O_OFF:R.O_OFF + dim][untouched])


@pytest.mark.parametrize("case", F.ex_cases(), ids=F.case_id)
def test_aggregate_ex_f16_stays_inside_the_fp32_kernels_bound(nn, case):
    """h contiguous fp16 (row stride = dim: odd dims read one column per lane, even ones two); `out` enters non-zero as a
    column block of a wider matrix whose other columns must not change; the in-degrees are added to a non-zero vector
    and equal bincount exactly.  The empty block launches nothing and changes nothing."""
    name, dim, weighted = case
    row, col, w, _, _ = F.structure(name)
    hbig, obig = F.tensors(dim, 0)
    h16 = F.h_of(hbig, dim, 0).contiguous()
    ref, S, k = F.aggregate_ref_f16(row.numpy(), col.numpy(), _np(w) if weighted else None, h16, F.NDST,
                                    out0=obig[:, R.O_OFF:R.O_OFF + dim].numpy())
    big = obig.cuda()
    before = big.clone()
    out = big[:, R.O_OFF:R.O_OFF + dim]
    deg = torch.full((F.NDST,), 3.0, device="cuda")
    nn.aggregate_into(out, h16.cuda(), row.cuda(), col.cuda(), w.cuda() if weighted else None, in_degree=deg)
    assert torch.equal(deg.cpu(), 3.0 + torch.from_numpy(k).float())
    _check_block(big, before, out, ref, S, k, dim, F.case_id(case))


@pytest.mark.parametrize("case", F.scaled_cases(), ids=F.case_id)
def test_aggregate_scaled_f16_stays_inside_the_fp32_kernels_bound(nn, case):
    """h is a column block of a wider fp16 matrix: the row stride exceeds dim and is even or odd, the base 4-byte
    aligned or not (f16_refs.H_FRAMES); every pair of degree modes occurs"""
    name, dim, frame, (src_mode, dst_mode), weighted = case
    row, col, w, src_deg, dst_deg = F.structure(name)
    hbig, obig = F.tensors(dim, frame)
    ref, S, k = F.aggregate_ref_f16(row.numpy(), col.numpy(), _np(w) if weighted else None, F.h_of(hbig, dim, frame),
                                    F.NDST, _np(src_deg) if src_mode else None, src_mode,
                                    _np(dst_deg) if dst_mode else None, dst_mode, obig[:, R.O_OFF:R.O_OFF + dim].numpy())
    big, dh = obig.cuda(), hbig.cuda()
    h = F.h_of(dh, dim, frame)
    assert h.stride(0) > dim and h.stride(0) % 2 == (dim + sum(F.H_FRAMES[frame])) % 2
    before = big.clone()
    out = big[:, R.O_OFF:R.O_OFF + dim]
    nn.aggregate_scaled_into(out, h, row.cuda(), col.cuda(), w.cuda() if weighted else None,
                             src_deg.cuda() if src_mode else None, src_mode, dst_deg.cuda() if dst_mode else None,
                             dst_mode)
    _check_block(big, before, out, ref, S, k, dim, F.case_id(case))


@pytest.mark.parametrize("frame", range(len(F.H_FRAMES)))
@pytest.mark.parametrize("dim", F.DIMS)
def test_f16_rows_equal_the_fp32_kernel_on_the_upcast_rows_bit_for_bit(nn, dim, frame):
    """train_refs.single_flush_block: every output element receives one atomic add, so nothing depends on the order
    between waves and the fp16 entry points must give exactly what the fp32 ones give for h.float() -- the same fp32
    products added in edge order.  All three ways in; the scaled one also with degree factors on both sides."""
    row, col, w = (t.cuda() for t in R.single_flush_block())
    g = torch.Generator().manual_seed(50 * dim + frame)
    left, right = F.H_FRAMES[frame]
    hbig = (torch.rand((R.EXACT_NSRC, left + dim + right), generator=g) * 3.5 - 1.75).half().cuda()
    h16 = hbig[:, left:left + dim]
    h32 = hbig.float()[:, left:left + dim]
    out0 = torch.randn((R.EXACT_NDST, dim + R.O_PAD), generator=g).cuda()
    sdeg = (torch.rand(R.EXACT_NSRC, generator=g) * 9).cuda()
    ddeg = (torch.rand(R.EXACT_NDST, generator=g) * 9).cuda()

    def both(fn):
        res = []
        for h in (h16, h32):
            big = out0.clone()
            fn(big[:, R.O_OFF:R.O_OFF + dim], h)
            res.append(big)
        assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32))
        assert not torch.equal(res[0], out0)

    both(lambda o, h: nn.aggregate_into(o, h.contiguous(), row, col, w))
    both(lambda o, h: nn.aggregate_into(o, h.contiguous(), row, col, None, in_degree=torch.zeros_like(ddeg)))
    both(lambda o, h: nn.aggregate_scaled_into(o, h, row, col, w, None, 0, None, 0))
    both(lambda o, h: nn.aggregate_scaled_into(o, h, row, col, w, sdeg, 1, ddeg, 2))
    a = nn.block_aggregate(h16.contiguous(), row, col, R.EXACT_NDST, edge_weight=w)
    b = nn.block_aggregate(h32.contiguous(), row, col, R.EXACT_NDST, edge_weight=w)
    assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("num_dst,din,pad", [(1, 4, 0), (77, 64, 4), (300, 128, 0), (513, 600, 8)])
def test_sage_finish_z_f16_is_exact(nn, num_dst, din, pad):
    """z[:, :din] = h[:num_dst] upcast (exact), the rest of the call as the fp32 entry point: z and inv equal, bit for
    bit, what fgnn_sage_finish_z gives for h.float(); h read out of a wider fp16 matrix when pad > 0"""
    g = torch.Generator().manual_seed(num_dst + din)
    hbig = torch.randn((num_dst + 9, din + pad), generator=g)
    hbig[1::5] *= 1e-6
    hbig = hbig.half().cuda()
    h16 = hbig[:, :din]
    z0 = torch.randn((num_dst, 2 * din + 4), generator=g).cuda()
    deg = torch.randint(0, 5, (num_dst,), generator=g).float().cuda()
    za, zb = z0.clone(), z0.clone()
    ia = nn.sage_finish_z(za, h16, deg, num_dst, din)
    ib = nn.sage_finish_z(zb, h16.float(), deg, num_dst, din)
    assert torch.equal(za.view(torch.int32), zb.view(torch.int32)) and torch.equal(ia, ib)
    assert torch.equal(za[:, :din], h16[:num_dst].float())
    assert torch.equal(za[:, 2 * din:], z0[:, 2 * din:])


def test_bad_arguments_are_refused_before_any_launch(hip):
    L = hip.load()
    E, dim = 40, 16
    row = torch.zeros(E, dtype=torch.int32, device="cuda")
    h = torch.ones((8, dim + 2), dtype=torch.float16, device="cuda")
    out = torch.zeros((4, dim), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    ex = lambda hp, d=dim: L.fgnn_block_aggregate_ex_f16(p(row), p(row), None, E, hp, d, p(out), dim, None, st)  # noqa: E731
    sc = lambda hp, ld: L.fgnn_block_aggregate_scaled_f16(p(row), p(row), None, E, hp, ld, dim, p(out), dim, None, 0,  # noqa: E731
                                                          None, 0, st)
    assert ex(p(h) + 1) == EINVAL and sc(p(h) + 1, dim + 2) == EINVAL      # an odd address
    assert sc(p(h), dim - 1) == EINVAL                                     # h_ld < dim
    assert ex(None) == EINVAL and ex(p(h), 0) == EINVAL
    assert L.fgnn_block_aggregate_scaled_f16(p(row), p(row), None, E, p(h), dim + 2, dim, p(out), dim - 1, None, 0,
                                             None, 0, st) == EINVAL        # out_ld < dim
    assert L.fgnn_block_aggregate_scaled_f16(p(row), p(row), None, E, p(h), dim + 2, dim, p(out), dim, None, 1,
                                             None, 0, st) == EINVAL        # a mode without its degree vector
    z = torch.zeros((4, 2 * dim), device="cuda")
    deg = torch.ones(4, device="cuda")
    fz = lambda hp, ld: L.fgnn_sage_finish_z_f16(p(z), 2 * dim, hp, ld, p(deg), p(deg), 4, dim, st)  # noqa: E731
    assert fz(p(h) + 2, dim + 2) == EINVAL and fz(p(h), dim + 2) == EINVAL and fz(p(h), dim - 4) == EINVAL
    torch.cuda.synchronize()
    assert not out.any() and not z.any()
    # an address that is 2- but not 4-byte aligned is fine: one column per lane
    assert sc(p(h) + 2, dim + 2) == 0 and ex(p(h) + 2) == 0
    torch.cuda.synchronize()
    assert float(out[0].sum()) == 2.0 * E * dim
