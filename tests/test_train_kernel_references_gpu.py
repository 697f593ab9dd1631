"""The training-side kernels (csrc/block_aggregate.hip, csrc/gnn_layers.hip, csrc/train_ops.hip; fgnn_hip/nn.py) and
fgnn_cache_table_replace against the float64 references of tests/train_refs.py, at the shapes where each kernel takes
another path: the template boundaries and the second and third `dbase` trip of the aggregation kernels, blocks smaller
than a wave's 32 edges, the second trip of every grid-stride loop (sizes from the device's CU count), both code paths
of softmax_xent with padded rows, the Philox mask of relu_dropout element by element.  tests/
test_train_kernel_references.py shows on the CPU that the references and bounds are sound.  Every test prints the
worst error / bound ratio before it asserts (pytest -s shows them; DESIGN.md 4.5 records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

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


@pytest.fixture(scope="module")
def cus(hip):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _structure(name):
    return tuple(t.cuda() for t in R.agg_structure(name))


# ---- A. aggregation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.agg_cases(), ids=R.case_id)
def test_aggregation_stays_inside_the_derived_bound(nn, case):
    """fgnn_block_aggregate_ex / fgnn_block_aggregate_scaled against aggregate_ref, |got - ref| <= (k + 8) 2^-23 S element
    by element, no atol.  `out` enters holding random values (the contract is +=) as a column block of a wider matrix
    whose other columns must not change by a bit; the scaled kernel reads h out of a wider matrix too
    (fgnn_block_aggregate_ex takes no row stride for h).  The unscaled kernel's in_degree output is added to a non-zero
    vector and must equal bincount(col) exactly."""
    name, dim, kernel, (src_mode, dst_mode), weighted = case
    args = R.agg_case_inputs(case)
    ref, S, k = R.aggregate_ref(**args)
    row, col, w, src_deg, dst_deg = _structure(name)
    hbig, obig = (t.cuda() for t in R.agg_tensors(name, dim))
    before = obig.clone()
    out = obig[:, R.O_OFF:R.O_OFF + dim]
    h = hbig[:, R.H_OFF:R.H_OFF + dim]
    if kernel == "ex":
        deg = torch.full((R.NDST,), 3.0, device="cuda")
        nn.aggregate_into(out, h.contiguous(), row, col, w if weighted else None, in_degree=deg)
        assert torch.equal(deg.cpu(), 3.0 + k.float())
    else:
        nn.aggregate_scaled_into(out, h, row, col, w if weighted else None, src_deg if src_mode else None, src_mode,
                                 dst_deg if dst_mode else None, dst_mode)
    R.assert_within(out, ref, R.aggregate_bound(S, k), R.case_id(case))
    assert torch.equal(obig[:, :R.O_OFF], before[:, :R.O_OFF])
    assert torch.equal(obig[:, R.O_OFF + dim:], before[:, R.O_OFF + dim:])
    assert torch.equal(out[(k == 0).cuda()], before[:, R.O_OFF:R.O_OFF + dim][(k == 0).cuda()])


@pytest.mark.parametrize("dim", R.EXACT_DIMS)
def test_aggregation_is_bit_exact_on_single_flush_blocks(nn, dim):
    """train_refs.single_flush_block: every output element receives exactly one atomic add, so all three ways into the
    aggregation kernel must equal sequential_f32 (products into the accumulator in edge order, one flush per segment,
    then onto out0) bit for bit -- a reordered or fused accumulation inside a wave does not.  `out` enters non-zero as a
    column block of a wider matrix, the scaled call reads h out of a wider matrix too; the in-degrees equal bincount."""
    row, col, w = R.single_flush_block()
    hbig, obig = R.exact_tensors(dim)
    h_cpu, out0 = hbig[:, R.H_OFF:R.H_OFF + dim], obig[:, R.O_OFF:R.O_OFF + dim]
    want = R.sequential_f32(row, col, w, h_cpu, out0).view(np.int32)
    drow, dcol, dw, dh = row.cuda(), col.cuda(), w.cuda(), hbig.cuda()
    h = dh[:, R.H_OFF:R.H_OFF + dim]

    def bits(t):
        return t.cpu().contiguous().numpy().view(np.int32)

    big = obig.cuda()
    deg = torch.zeros(R.EXACT_NDST, device="cuda")
    nn.aggregate_into(big[:, R.O_OFF:R.O_OFF + dim], h.contiguous(), drow, dcol, dw, in_degree=deg)
    assert np.array_equal(bits(big[:, R.O_OFF:R.O_OFF + dim]), want)
    assert torch.equal(deg.cpu(), torch.bincount(col.long(), minlength=R.EXACT_NDST).float())
    keep = torch.ones(dim + R.O_PAD, dtype=torch.bool)
    keep[R.O_OFF:R.O_OFF + dim] = False
    assert np.array_equal(bits(big[:, keep.cuda()]), bits(obig[:, keep]))

    big = obig.cuda()
    nn.aggregate_scaled_into(big[:, R.O_OFF:R.O_OFF + dim], h, drow, dcol, dw, None, 0, None, 0)
    assert np.array_equal(bits(big[:, R.O_OFF:R.O_OFF + dim]), want)
    assert np.array_equal(bits(big[:, keep.cuda()]), bits(obig[:, keep]))

    got = nn.block_aggregate(h.contiguous(), drow, dcol, R.EXACT_NDST, edge_weight=dw)
    assert np.array_equal(bits(got), R.sequential_f32(row, col, w, h_cpu, None).view(np.int32))


@pytest.mark.parametrize("dim", R.BACKWARD_DIMS)
def test_block_aggregate_backward_is_the_reference_with_the_roles_swapped(nn, dim):
    """_BlockAggregate under autograd: the output against aggregate_ref, the input gradient against aggregate_ref with
    row and col swapped (k = the edge count of every SOURCE), same bound"""
    row, col, w, h, gout = R.backward_inputs(dim)
    hh = h.cuda().requires_grad_()
    out = nn.block_aggregate(hh, row.cuda(), col.cuda(), R.NDST, edge_weight=w.cuda())
    out.backward(gout.cuda())
    ref, S, k = R.aggregate_ref(row, col, w, h, R.NDST)
    R.assert_within(out, ref, R.aggregate_bound(S, k), "forward %d" % dim)
    ref, S, k = R.aggregate_ref(col, row, w, gout, R.NSRC)
    R.assert_within(hh.grad, ref, R.aggregate_bound(S, k), "backward %d" % dim)
    assert not hh.grad[(k == 0).cuda()].any()


@pytest.mark.parametrize("name", R.DEGREE_STRUCTS)
def test_in_degree_and_block_degrees(nn, name):
    """in_degree of fgnn_block_aggregate_ex (run-head ballot over 32-edge chunks) and both vectors of fgnn_block_degrees
    (64-edge waves): counts equal bincount exactly, on a zeroed and on a non-zero vector; the weight sums of non-integer
    weights satisfy |got - ref| <= (k + 2) 2^-23 sum|w|"""
    row, col, w, _, _ = _structure(name)
    k = torch.bincount(col.long().cpu(), minlength=R.NDST).float()
    h = torch.ones((R.NSRC, 1), device="cuda")
    for start in (0.0, 5.0):
        deg = torch.full((R.NDST,), start, device="cuda")
        out = nn.aggregate_into(torch.zeros((R.NDST, 1), device="cuda"), h, row, col, None, in_degree=deg)
        assert torch.equal(deg.cpu(), start + k) and torch.equal(out.cpu().flatten(), k)
    src_deg, dst_deg = nn.block_degrees(row, col, R.NSRC, R.NDST)
    assert torch.equal(dst_deg.cpu(), k)
    assert torch.equal(src_deg.cpu(), torch.bincount(row.long().cpu(), minlength=R.NSRC).float())
    src_deg, dst_deg = nn.block_degrees(row, col, R.NSRC, R.NDST, edge_weight=w)
    ref, s_abs, kk = R.degrees_ref(col.cpu(), w.cpu(), R.NDST)
    R.assert_within(dst_deg, ref, R.degrees_bound(s_abs, kk), "weighted degrees " + name)
    assert torch.equal(src_deg.cpu(), torch.bincount(row.long().cpu(), minlength=R.NSRC).float())
    assert not dst_deg[(kk == 0).cuda()].any()


# ---- B. relu_dropout --------------------------------------------------------------------------------------------------------

SEED = 0xDEADBEEF12345678
P_SMALL = 2.0 ** -20


def _dropout_both_ways(nn, x_cpu, p, step, tag):
    x = x_cpu.cuda().requires_grad_()
    d_step = None if step is None else torch.tensor([step, 0], dtype=torch.int64, device="cuda")
    y = nn.relu_dropout(x, p, True, seed=SEED, d_step=d_step, tag=tag)
    want = R.dropout_ref(x_cpu.numpy(), p, SEED, step or 0, tag)
    got = y.detach().cpu().numpy()
    assert np.array_equal(got, want), (p, step, tag, int((got != want).sum()))
    gy = torch.randn(x_cpu.shape, generator=torch.Generator().manual_seed(9))
    (gx,) = torch.autograd.grad(y, x, gy.cuda())
    want_g = np.where(want > 0, gy.numpy() * R.dropout_scale(p), np.float32(0)).astype(np.float32)
    assert np.array_equal(gx.cpu().numpy(), want_g), (p, step, tag)
    return want


@pytest.mark.parametrize("n", [4, 1028])
def test_relu_dropout_equals_the_philox_reference_element_by_element(nn, n):
    """y == dropout_ref(x) for every p, step count (absent, 3, 2^32 + 3: the high word goes into the key) and tag, a
    seed with high bits set; the backward pass == where(y > 0, gy * scale, 0)"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    seen = set()
    for p in (0.1, 0.5, 0.9, P_SMALL):
        for step in (None, 3, 2 ** 32 + 3):
            for tag in (0, 5):
                want = _dropout_both_ways(nn, x, p, step, tag)
                if p != P_SMALL:  # (p = 2^-20 drops next to nothing: its masks coincide)
                    seen.add(want.tobytes())
    if n > 4:
        assert len(seen) == 3 * 3 * 2  # every (p, step, tag) drew another mask


@pytest.mark.parametrize("p,step,tag", [(0.5, None, 0), (0.1, 2 ** 32 + 3, 5), (0.9, 3, 5), (P_SMALL, 3, 0)])
def test_relu_dropout_past_the_grid_cap(nn, cus, p, step, tag):
    """more float4s than 16 x CUs workgroups of 256 threads hold, plus an odd tail: the stride loops of the forward and
    the backward kernel take a second trip (about 17 MB on 256 CUs)"""
    n4 = 16 * cus * 256 + 257
    x = torch.randn(4 * n4, generator=torch.Generator().manual_seed(12))
    want = _dropout_both_ways(nn, x, p, step, tag)
    kept = float((want != 0).sum()) / float((x > 0).sum())
    assert abs(kept - (1 - p)) < 0.002, kept


def test_relu_dropout_refuses_bad_arguments_and_leaves_the_output(hip):
    L = hip.load()
    x = torch.ones(8, device="cuda")
    y = torch.full((8,), 777.0, device="cuda")
    for n, p in ((8, 1.0), (8, -0.25), (6, 0.5), (8, float("nan"))):
        assert L.fgnn_relu_dropout(_p(x), _p(y), C.c_size_t(n), C.c_float(p), C.c_uint64(1), None, C.c_uint32(0),
                                   _st()) == EINVAL, (n, p)
        assert L.fgnn_relu_dropout_backward(_p(x), _p(x), _p(y), C.c_size_t(n), C.c_float(p), _st()) == EINVAL, (n, p)
    torch.cuda.synchronize()
    assert bool((y == 777.0).all())
    assert L.fgnn_relu_dropout(_p(x), _p(y), C.c_size_t(8), C.c_float(0.0), C.c_uint64(1), None, C.c_uint32(0), _st()) == 0
    assert torch.equal(y, x)  # p = 0 keeps every element, scale 1


# ---- C. softmax_xent ----------------------------------------------------------------------------------------------------------

def _xent(L, c, n, ws):
    """one launch through the C ABI with ld = c + 3 and dl_ld = c + 5; -> (loss, dlogits [n, c], padding intact)"""
    x, y = R.xent_inputs(c, n)
    xb = torch.full((n, c + 3), 1e30, device="cuda")  # a kernel that read the padding as logits would not survive it
    xb[:, :c] = x.cuda()
    gb = torch.full((n, c + 5), 777.0, device="cuda")
    loss = torch.full((), 777.0, device="cuda")
    y = y.cuda()
    code = L.fgnn_softmax_xent(_p(xb), C.c_size_t(c + 3), _p(y), C.c_size_t(n), C.c_size_t(c), _p(loss), _p(gb),
                               C.c_size_t(c + 5), _p(ws), C.c_size_t(ws.numel() * 4), _st())
    assert code == 0
    return loss.cpu(), gb[:, :c].cpu(), bool((gb[:, c:] == 777.0).all())


@pytest.mark.parametrize("c", R.XENT_C)
def test_softmax_xent_against_float64_reference(hip, c):
    """loss and gradient against xent_ref for n = 5, 2500 (more than 512 workgroups x 4 rows: the row loop strides), 5
    again and 1 on ONE scratch buffer (the kernel restores its arrival counter), padded rows on both sides, labels 0,
    c - 1, -100 and c, rows N(0, 3) / all equal / +80 among -80s at and off the label / -inf off the label.
    |loss - ref| <= 4 d_loss + 2^-22 |ref| and |grad - ref| <= 4 max(d_grad) + 2^-24 / n_valid, d = the deviation of
    torch's fp32 cross_entropy from the reference (d_grad per row, its maximum over the rows: train_refs.
    xent_expectation).  Observed on an MI355X (worst over all c and n): loss error / bound 0.90 (C = 2, n = 5; 0.49 at most for n = 2500),
    gradient error / bound 0.44; at n = 2500 the kernel's largest gradient deviation is 0.5 - 1.2 x torch's (DESIGN.md
    4.5)."""
    L = hip.load()
    ws = torch.zeros((L.fgnn_softmax_xent_scratch_bytes(C.c_size_t(2500)) + 3) // 4, dtype=torch.int32, device="cuda")
    for n in (5, 2500, 5, 1):
        ref_loss, ref_grad, b_loss, b_grad, d_loss, d_grad = R.xent_expectation(c, n)
        loss, grad, pad_ok = _xent(L, c, n, ws)
        y = R.xent_inputs(c, n)[1]
        print("C=%d n=%d: torch fp32 d_loss %.3g, kernel %.3g; torch max d_grad %.3g, kernel %.3g" % (
            c, n, float(d_loss), abs(float(loss) - float(ref_loss)), float(d_grad.max()),
            float((grad.double() - ref_grad).abs().max())))
        R.assert_within(loss, ref_loss, b_loss, "loss C=%d n=%d" % (c, n))
        R.assert_within(grad, ref_grad, b_grad, "grad C=%d n=%d" % (c, n))
        assert pad_ok and not grad[(y < 0) | (y >= c)].any()
        assert int(ws[0]) == 0


# ---- D. Adam ------------------------------------------------------------------------------------------------------------------

def _report_adam(what, got, ref, bound, dev):
    worst, k_dev, t_dev = 0.0, 0.0, 0.0
    for g, r, b, d in zip(got, ref, bound, dev):
        if r.numel():
            worst = max(worst, R.worst_ratio(g, r, b))
            k_dev, t_dev = max(k_dev, float((g.detach().cpu().double() - r).abs().max())), max(t_dev, d)
    print("%s: torch fp32 deviation %.3g, kernel %.3g, worst error / bound %.4g" % (what, t_dev, k_dev, worst))
    return worst


@pytest.mark.parametrize("wd", R.ADAM_WD)
@pytest.mark.parametrize("name", R.ADAM_SETS)
def test_adam_against_float64_reference(nn, cus, name, wd):
    """four steps from zero parameters (their values stay the size of the updates, lr = 0.1) with N(0, 1) gradients and
    float32-representable hyperparameters; after every step, per tensor, |nn.Adam - adam_ref| <= 4 max|torch fp32 -
    adam_ref| + 2^-24 max|ref|.  8 tensors (one launch), 9 and 17 (two and three), one tensor past the 8 x CUs
    workgroups of the stride loop, a set whose largest tensor comes last.  With the bias corrections in fp32 (1 -
    powf(b2, step)) the worst error / bound on an MI355X was 4.0 (step 2; 1.7 - 4.0 from step 2 on in every set, the
    kernel's deviation ten times torch's); computed in double it is 0.42, the deviations equal."""
    grads, ref, bound, dev = R.adam_expectation(name, cus, wd)
    qs = [torch.zeros(g.shape, device="cuda").requires_grad_() for g in grads[0]]
    opt = nn.Adam(qs, weight_decay=wd, **R.ADAM)
    worst = []
    for step in range(R.ADAM_STEPS):
        for q, g in zip(qs, grads[step]):
            q.grad = g.cuda()
        opt.step()
        worst.append(_report_adam("%s wd=%g step %d" % (name, wd, step + 1), qs, ref[step], bound[step], dev[step]))
    assert int(opt.step_count[0]) == R.ADAM_STEPS
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("null_pointers", [False, True])
def test_adam_with_a_zero_length_tensor_through_the_c_abi(hip, cus, null_pointers):
    """a tensor of no elements among others (torch hands out a null data pointer for it, or the caller passes any
    pointer): the others are updated like the reference's, nothing is written through the empty one's pointers"""
    L = hip.load()
    wd = R.ADAM_WD[1]
    grads, ref, bound, dev = R.adam_expectation("zero_length", cus, wd)
    guard = torch.full((64,), 777.0, device="cuda")
    ps = [torch.zeros(g.shape, device="cuda") for g in grads[0]]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    d_step = torch.zeros(2, dtype=torch.int64, device="cuda")

    def arr(ts):
        return (C.c_void_p * 3)(*[t.data_ptr() if t.numel() else (0 if null_pointers else guard.data_ptr()) for t in ts])

    lr, (b1, b2), eps = R.ADAM["lr"], R.ADAM["betas"], R.ADAM["eps"]
    worst = []
    for step in range(R.ADAM_STEPS):
        gs = [g.cuda() for g in grads[step]]
        numel = (C.c_size_t * 3)(*[p.numel() for p in ps])
        code = L.fgnn_adam_step(arr(ps), arr(gs), arr(ms), arr(vs), numel, C.c_int(3), C.c_float(lr), C.c_float(b1),
                                C.c_float(b2), C.c_float(eps), C.c_float(wd), _p(d_step), _st())
        assert code == 0
        worst.append(_report_adam("zero_length step %d" % (step + 1), ps, ref[step], bound[step], dev[step]))
    assert int(d_step[0]) == R.ADAM_STEPS and int(d_step[1]) == 0
    assert bool((guard == 777.0).all())
    assert max(worst) <= 1.0, worst


# ---- E. relu_l2norm and the SAGE elementwise pair ----------------------------------------------------------------------------

@pytest.mark.parametrize("dim", R.L2_DIMS)
def test_relu_l2norm_against_float64_reference(hip, nn, cus, dim):
    """8 x CUs x 4 + 5 rows (the row loop of both kernels takes a second trip), dim 7 and 300 (wider than the 256
    columns a wave keeps in registers); x, out, gout and gx are column blocks of wider matrices whose other columns must
    not change.  Rows without a positive entry: exactly 0 out, exactly 0 gradient, inv_norm exactly 1.  Bound: 4 x the
    torch fp32 formulation's deviation from the reference (forward: of the row; backward: of the tensor, see
    train_refs.l2norm_expectation) + 2^-22 |ref|.  Observed on an MI355X: forward error / bound 0.53 (dim 7) and 0.42
    (dim 300), backward 0.43 and 0.17."""
    L = hip.load()
    rows = R.l2norm_rows(cus)
    y_ref, inv_ref, gx_ref, b_y, b_gx, d_y, d_gx = R.l2norm_expectation(dim, rows)
    xbig, gbig = (t.cuda() for t in R.l2norm_inputs(dim, rows))
    x, gout = xbig[:, R.X_OFF:R.X_OFF + dim], gbig[:, R.G_OFF:R.G_OFF + dim]
    obig = torch.full((rows, dim + 4), 777.0, device="cuda")
    gxbig = torch.full((rows, dim + 7), 777.0, device="cuda")
    out, gx = obig[:, 1:1 + dim], gxbig[:, 4:4 + dim]
    inv = torch.full((rows,), 777.0, device="cuda")
    assert L.fgnn_relu_l2norm(_p(x), C.c_size_t(dim + R.X_PAD), _p(out), C.c_size_t(dim + 4), _p(inv), C.c_size_t(rows),
                              C.c_size_t(dim), _st()) == 0
    assert L.fgnn_relu_l2norm_backward(_p(out), C.c_size_t(dim + 4), _p(inv), _p(gout), C.c_size_t(dim + R.G_PAD),
                                       _p(gx), C.c_size_t(dim + 7), C.c_size_t(rows), C.c_size_t(dim), _st()) == 0
    print("dim %d: torch fp32 max deviation forward %.3g backward %.3g; kernel %.3g / %.3g" % (
        dim, float(d_y.max()), float(d_gx.max()), float((out.cpu().double() - y_ref).abs().max()),
        float((gx.cpu().double() - gx_ref).abs().max())))
    R.assert_within(out, y_ref, b_y, "relu_l2norm forward, dim %d" % dim)
    R.assert_within(gx, gx_ref, b_gx, "relu_l2norm backward, dim %d" % dim)
    assert not out[::10].any() and not gx[::10].any() and bool((inv[::10] == 1.0).all())
    assert bool((inv[1::10] > 0).all()) and bool(out[1].any())
    assert bool((obig[:, 0] == 777.0).all()) and bool((obig[:, 1 + dim:] == 777.0).all())
    assert bool((gxbig[:, :4] == 777.0).all()) and bool((gxbig[:, 4 + dim:] == 777.0).all())
    # the autograd wrapper runs the same two launches
    xx = xbig.clone().requires_grad_()
    y2 = nn.relu_l2norm(xx[:, R.X_OFF:R.X_OFF + dim])
    y2.backward(gout)
    assert torch.equal(y2.detach(), out) and torch.equal(xx.grad[:, R.X_OFF:R.X_OFF + dim], gx)
    assert not xx.grad[:, :R.X_OFF].any() and not xx.grad[:, R.X_OFF + dim:].any()


def test_sage_finish_z_and_grad_prep_past_the_grid_cap_with_row_strides(nn, cus):
    """equality with the torch formulation, as tests/test_train_ops_gpu.py, at a size with more float4s than 16 x CUs
    workgroups of 256 threads hold (20 011 x 256 on 256 CUs) and with z, h and gz as column blocks of wider matrices;
    degrees include 0, values below 1 and non-integers"""
    din = 256
    num_dst = 16 * cus * 256 // (din // 4) + 3627
    num_src = num_dst + 9
    g = torch.Generator(device="cuda").manual_seed(2)
    zbig = torch.randn((num_dst, 2 * din + 8), generator=g, device="cuda")
    hbig = torch.randn((num_src, din + 8), generator=g, device="cuda")
    gzbig = torch.randn((num_dst, 2 * din + 12), generator=g, device="cuda")
    z, h, gz = zbig[:, 4:4 + 2 * din], hbig[:, 4:4 + din], gzbig[:, 8:8 + 2 * din]
    deg = torch.randint(0, 5, (num_dst,), generator=g, device="cuda").float()
    deg[::3] += 0.5
    want_inv = deg.clamp(min=1).reciprocal()
    want = zbig.clone()
    want[:, 4 + din:4 + 2 * din] *= want_inv.unsqueeze(1)
    want[:, 4:4 + din] = h[:num_dst]
    inv = nn.sage_finish_z(z, h, deg, num_dst, din)
    assert torch.equal(inv, want_inv) and torch.equal(zbig, want)
    gh, gagg = nn.sage_grad_prep(gz, inv, num_src, din)
    assert torch.equal(gagg, gz[:, din:] * inv.unsqueeze(1))
    want_gh = torch.zeros((num_src, din), device="cuda")
    want_gh[:num_dst] = gz[:, :din]
    assert torch.equal(gh, want_gh)


# ---- F. fgnn_cache_table_replace -------------------------------------------------------------------------------------------------

def _u32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


@pytest.mark.parametrize("case", R.CACHE_CASES, ids=lambda c: "%d-%d-%d" % c[:3])
def test_cache_table_replace_against_numpy(hip, case):
    """old nodes -> EMPTY, then new node i -> i, on a table built by fgnn_cache_table_build; the lists overlap in part
    (a node in both ends with its new position), every other entry is unchanged.  A table of 50 000 entries cannot hold
    70 001 distinct ids: see train_refs.CACHE_CASES."""
    num_node, n_old, n_new, _ = case
    rank, num_cached, old, new = R.cache_replace_inputs(*case)
    table = hip.cache_table_build(_u32(rank), num_cached, num_node)
    t0 = table.cpu().numpy().view(np.uint32).copy()
    built = np.full(num_node, R.EMPTY, dtype=np.uint32)
    built[rank[:num_cached]] = np.arange(num_cached, dtype=np.uint32)
    assert np.array_equal(t0, built)
    hip.cache_table_replace(table, _u32(old) if n_old else None, _u32(new))
    got = table.cpu().numpy().view(np.uint32)
    want = R.cache_replace_ref(t0, old, new)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, t0)
