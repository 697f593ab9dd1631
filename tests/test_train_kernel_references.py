"""The references and bounds of tests/train_refs.py are sound, shown on the CPU before any kernel is held to them
(tests/test_train_kernel_references_gpu.py): the numpy Philox is the oracle's word for word, the float64 references
agree with torch's float64 ops, and an honest fp32 implementation (torch on the CPU) passes every derived bound on the
very inputs the GPU tests use, with no slack added."""
import numpy as np
import pytest
import torch

import train_refs as R

CUS = 256  # stands in for the chip's CU count where a size depends on it (the GPU tests ask the device)


def test_philox_blocks_equal_the_oracle_word_for_word(oracle):
    rs = np.random.default_rng(5)
    for i in range(1000):
        seed = int(rs.integers(0, 2 ** 64, dtype=np.uint64)) if i % 2 else int(rs.integers(0, 2 ** 32))
        step = int(rs.integers(0, 2 ** 64, dtype=np.uint64)) if i % 3 == 0 else int(rs.integers(0, 2 ** 33))
        tag = int(rs.integers(0, 2 ** 32)) if i % 5 == 0 else int(rs.integers(0, 8))
        t = int(rs.integers(0, 2 ** 40)) if i % 4 == 0 else int(rs.integers(0, 2 ** 22))
        got = R.philox_blocks(seed, step, tag, 3, first=t)
        for j in range(3):
            want = oracle.philox_draw(seed, step, tag, (t + j) & 0xFFFFFFFF, (t + j) >> 32)
            assert got[j].tolist() == want, (seed, step, tag, t + j)
    # consecutive blocks from 0, as dropout_ref uses them
    got = R.philox_blocks(0xDEADBEEF12345678, 2 ** 32 + 3, 5, 64)
    assert got.dtype == np.uint32 and got.shape == (64, 4)
    for t in range(64):
        assert got[t].tolist() == oracle.philox_draw(0xDEADBEEF12345678, 2 ** 32 + 3, 5, t, 0)


def test_philox_blocks_known_answers():
    """Random123 kat_vectors for philox4x32-10 (tests/test_oracle_golden.py), through philox_blocks' addressing:
    counter (t >> 32, lo32(t), tag, lo32(step)), key (lo32(seed), hi32(seed) ^ hi32(step))"""
    for ctr, key, want in (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
                            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        t = (ctr[0] << 32) | ctr[1]
        for hi_step in (0, 0x5555AAAA):  # the key's high word is split between seed and step
            seed = key[0] | ((key[1] ^ hi_step) << 32)
            step = ctr[3] | (hi_step << 32)
            assert R.philox_blocks(seed, step, ctr[2], 1, first=t)[0].tolist() == want


def test_dropout_ref_threshold_and_scale():
    x = np.linspace(-1, 1, 4096, dtype=np.float32)
    for p in (0.1, 0.5, 0.9, 2.0 ** -20):
        y = R.dropout_ref(x, p, 7, 0, 0)
        words = R.philox_blocks(7, 0, 0, 1024).reshape(-1)
        keep = words >= int(float(np.float32(p)) * 2 ** 32)
        assert np.array_equal(y != 0, keep & (x > 0))
        assert np.array_equal(y[y != 0], (x * R.dropout_scale(p))[y != 0]) and y.dtype == np.float32
        assert abs(keep.mean() - (1 - p)) < 0.03
    assert np.array_equal(R.dropout_ref(x, 0.0, 7, 0, 0), np.maximum(x, 0))


@pytest.mark.parametrize("case", R.agg_cases(), ids=R.case_id)
def test_fp32_aggregation_stays_inside_the_derived_bound(case):
    """torch's CPU fp32 formulation (index_add_ of the fp32 products, times the fp32 factor) on every aggregation input
    of the GPU test: a condition on the inputs and the bound, no slack"""
    args = R.agg_case_inputs(case)
    ref, S, k = R.aggregate_ref(**args)
    assert torch.equal(k, torch.bincount(args["col"].long(), minlength=R.NDST))
    R.assert_within(R.aggregate_fp32(**args), ref, R.aggregate_bound(S, k), R.case_id(case))
    # the bound is not vacuous: it is far below the result's size, and an output without an edge must keep out0
    assert float((R.aggregate_bound(S, k) / S).max()) < 1e-3
    assert torch.equal(ref[k == 0], args["out0"][k == 0].double())


def test_aggregation_cases_cover_what_they_claim():
    cases = R.agg_cases()
    assert len(cases) < 100
    pairs = {(c[0], c[1]) for c in cases}
    for name in R.AGG_STRUCTS:
        assert len({d for n, d in pairs if n == name}) >= 2, name
    for dim in R.AGG_DIMS:
        assert len({n for n, d in pairs if d == dim}) >= 2, dim
    assert {c[3] for c in cases if c[2] == "scaled"} == set(R.SCALED_MODES)
    sizes = {name: R.agg_structure(name)[0].numel() for name in R.AGG_STRUCTS}
    assert [sizes[n] for n in ("e1", "e31", "e32", "e33", "e127", "e128", "e129", "one_dst", "own_dst")] == \
        [1, 31, 32, 33, 127, 128, 129, 4099, 300] and sizes["fused_sorted"] == sizes["fused_permuted"] == 6001
    row, col, w, src_deg, dst_deg = R.agg_structure("fused_sorted")
    assert bool(((dst_deg > 0) & (dst_deg < 1)).any())        # the clamp on a non-zero degree
    used = src_deg[row.long()]
    assert bool((used == 0).any()) and bool((used != used.round()).any())  # referenced sources: degree 0, non-integer
    assert bool((w != w.round()).all()) and float(w.max()) < 1.5 and float(w.min()) > 0
    assert bool((torch.sort(col)[0] == col).all()) and not bool((torch.sort(R.agg_structure("fused_permuted")[1])[0] ==
                                                                R.agg_structure("fused_permuted")[1]).all())
    col = R.agg_structure("runs")[1]
    assert (col[64:96] == 200).all() and col[63] != 200 and col[96] != 200    # exactly one 32-edge chunk
    assert (col[31:41] == 50).all() and col[30] != 50 and col[41] != 50      # starts on a chunk's last lane
    assert (col[128:192] == 250).all() and col[127] != 250 and col[192] != 250


def test_single_flush_block_respects_the_chunk_rule_and_its_reference_the_bound():
    """every destination owns one contiguous run, no run crosses a multiple of 32 in the edge array, run lengths 1 to 32
    all occur, the last chunk is short and no multiple of 4; sequential_f32 on it lies inside aggregate_bound of
    aggregate_ref (it is one of the orders the bound covers)"""
    row, col, w = R.single_flush_block()
    c = col.numpy()
    heads = np.flatnonzero(np.r_[True, c[1:] != c[:-1]])
    ends = np.r_[heads[1:], c.size]
    assert len(set(c[heads].tolist())) == heads.size == len(R.EXACT_RUNS) < R.EXACT_NDST  # one run per destination
    assert (ends - heads).tolist() == list(R.EXACT_RUNS) and set(R.EXACT_RUNS) == set(range(1, 33))
    assert (heads // R.EXACT_CHUNK == (ends - 1) // R.EXACT_CHUNK).all()
    assert 0 < c.size % R.EXACT_CHUNK and (c.size % R.EXACT_CHUNK) % 4 != 0
    assert int(row.min()) == 0 and int(row.max()) == R.EXACT_NSRC - 1
    assert bool((w != w.round()).all()) and float(w.min()) >= 0.25
    for dim in (1, 65):
        hbig, obig = R.exact_tensors(dim)
        h, out0 = hbig[:, R.H_OFF:R.H_OFF + dim], obig[:, R.O_OFF:R.O_OFF + dim]
        assert float(hbig.abs().min()) >= 0.25 and float(obig.abs().min()) >= 0.25
        got = R.sequential_f32(row, col, w, h, out0)
        assert got.dtype == np.float32
        ref, S, k = R.aggregate_ref(row, col, w, h, R.EXACT_NDST, out0=out0)
        R.assert_within(torch.from_numpy(got), ref, R.aggregate_bound(S, k), "sequential fp32, dim %d" % dim)
        assert np.array_equal(got[k.numpy() == 0], out0.numpy()[k.numpy() == 0])
        zero = R.sequential_f32(row, col, None, h, None)
        ref, S, k = R.aggregate_ref(row, col, None, h, R.EXACT_NDST)
        R.assert_within(torch.from_numpy(zero), ref, R.aggregate_bound(S, k), "sequential fp32 unweighted, dim %d" % dim)


@pytest.mark.parametrize("dim", R.BACKWARD_DIMS)
def test_fp32_aggregation_backward_stays_inside_the_derived_bound(dim):
    row, col, w, h, gout = R.backward_inputs(dim)
    ref, S, k = R.aggregate_ref(col, row, w, gout, R.NSRC)
    R.assert_within(R.aggregate_fp32(col, row, w, gout, R.NSRC), ref, R.aggregate_bound(S, k), "backward %d" % dim)


@pytest.mark.parametrize("name", R.DEGREE_STRUCTS)
def test_fp32_weighted_degrees_stay_inside_the_derived_bound(name):
    _, col, w, _, _ = R.agg_structure(name)
    ref, s_abs, k = R.degrees_ref(col, w, R.NDST)
    got = torch.zeros(R.NDST).index_add_(0, col.long(), w)
    R.assert_within(got, ref, R.degrees_bound(s_abs, k), "degrees " + name)


@pytest.mark.parametrize("c", R.XENT_C)
@pytest.mark.parametrize("n", R.XENT_N)
def test_xent_ref_agrees_with_float64_cross_entropy(c, n):
    x, y = R.xent_inputs(c, n)
    assert int(y[0]) == 0 and (n == 1 or int(y[1]) == c - 1)
    if n > 1:
        assert bool((y == -100).any()) and bool((y == c).any())
    loss, grad = R.xent_ref(x, y)
    want, want_g = R.xent_torch(x, y, torch.float64)
    assert abs(float(loss) - float(want)) <= 1e-12 and float((grad - want_g).abs().max()) <= 1e-12
    assert not grad[(y < 0) | (y >= c)].any() and bool(torch.isfinite(grad).all()) and np.isfinite(float(loss))
    # the measured tolerance is finite and small against the values it guards
    _, _, b_loss, b_grad, _, _ = R.xent_expectation(c, n)
    assert float(b_loss) <= 1e-5 * max(float(loss.abs()), 1.0) and float(b_grad.max()) * max(n, 1) <= 1e-5


@pytest.mark.parametrize("c", R.XENT_C)
@pytest.mark.parametrize("n", R.XENT_N)
def test_fp32_one_pass_xent_stays_inside_the_measured_bound(c, n):
    """the bound is measured on torch's log_softmax + nll_loss; the kernel's one-pass formulation in honest fp32 on the
    CPU must pass it too, or the bound would judge the formulation, not the kernel"""
    ref_loss, ref_grad, b_loss, b_grad, _, _ = R.xent_expectation(c, n)
    loss, grad = R.xent_fp32_one_pass(*R.xent_inputs(c, n))
    R.assert_within(loss, ref_loss, b_loss, "one-pass fp32 loss C=%d n=%d" % (c, n))
    R.assert_within(grad, ref_grad, b_grad, "one-pass fp32 grad C=%d n=%d" % (c, n))


@pytest.mark.parametrize("name", R.ADAM_SETS + ("zero_length",))
@pytest.mark.parametrize("wd", R.ADAM_WD)
def test_adam_ref_agrees_with_float64_torch_adam(name, wd):
    grads = R.adam_grads(name, CUS)
    assert len(grads) == R.ADAM_STEPS
    ref = R.adam_ref(grads, weight_decay=wd, **R.ADAM)
    want = R.adam_torch(grads, weight_decay=wd, dtype=torch.float64, **R.ADAM)
    for r_s, w_s in zip(ref, want):
        for r, t in zip(r_s, w_s):
            assert r.shape == t.shape and (not r.numel() or float((r - t).abs().max()) <= 1e-12)
    if name == "stride":
        assert grads[0][0].numel() > 8 * CUS * 256
    # the measured tolerance is a few fp32 ulp of the parameters (size ~ lr per step), not more
    _, _, bound, _ = R.adam_expectation(name, CUS, wd)
    for b_s, r_s in zip(bound, ref):
        for b, r in zip(b_s, r_s):
            assert not r.numel() or float(b) <= 64 * 2.0 ** -24 * float(r.abs().max())


def test_adam_hyperparameters_are_float32_numbers():
    for v in (R.ADAM["lr"], *R.ADAM["betas"], R.ADAM["eps"], *R.ADAM_WD):
        assert float(np.float32(v)) == v


@pytest.mark.parametrize("dim", R.L2_DIMS)
def test_relu_l2norm_ref_agrees_with_float64_autograd(dim):
    rows = 203
    xbig, gbig = R.l2norm_inputs(dim, rows)
    x, gout = xbig[:, R.X_OFF:R.X_OFF + dim].double(), gbig[:, R.G_OFF:R.G_OFF + dim].double()
    y, inv, gx = R.relu_l2norm_ref(x, gout)
    xx = x.clone().requires_grad_()
    z = torch.relu(xx)
    n = z.norm(2, 1, keepdim=True)
    want = z / torch.where(n == 0, torch.ones_like(n), n)
    (want_g,) = torch.autograd.grad(want, xx, gout)
    want = want.detach()
    assert float((y - want).abs().max()) <= 1e-12 and float((gx - want_g).abs().max()) <= 1e-11
    assert not y[::10].any() and not gx[::10].any() and bool((inv[::10] == 1).all()) and bool(y[1].any())


@pytest.mark.parametrize("dim", R.L2_DIMS)
def test_fp32_relu_l2norm_in_the_kernels_formulation_stays_inside_the_measured_bound(dim):
    """the bound is measured on the op-by-op torch formulation; the kernel's own formulation (gx from the rounded y and
    inv_norm) in honest fp32 on the CPU must pass it too, or the bound would judge the formulation, not the kernel"""
    rows = R.l2norm_rows(CUS)
    xbig, gbig = R.l2norm_inputs(dim, rows)
    y, inv, gx, b_y, b_gx, _, _ = R.l2norm_expectation(dim, rows)
    y32, _, gx32 = R.relu_l2norm_ref(xbig[:, R.X_OFF:R.X_OFF + dim], gbig[:, R.G_OFF:R.G_OFF + dim], torch.float32)
    R.assert_within(y32, y, b_y, "relu_l2norm fp32 forward, dim %d" % dim)
    R.assert_within(gx32, gx, b_gx, "relu_l2norm fp32 backward, dim %d" % dim)


@pytest.mark.parametrize("case", R.CACHE_CASES, ids=lambda c: "%d-%d-%d" % c[:3])
def test_cache_replace_inputs_and_reference(case):
    num_node, n_old, n_new, distinct = case
    rank, num_cached, old, new = R.cache_replace_inputs(*case)
    assert old.size == n_old and new.size == n_new and len(set(new.tolist())) == n_new
    assert (len(set(old.tolist())) == n_old) == (distinct or n_old == 0)
    if n_old > 1 and n_new > 1:
        both = np.intersect1d(old, new)
        assert 0 < both.size < min(n_old, n_new) or not distinct
    table = np.full(num_node, R.EMPTY, dtype=np.uint32)
    table[rank[:num_cached]] = np.arange(num_cached, dtype=np.uint32)
    got = R.cache_replace_ref(table, old, new)
    assert (got[new] == np.arange(n_new)).all()
    gone = np.setdiff1d(old, new)
    assert (got[gone] == R.EMPTY).all()
    rest = np.setdiff1d(np.arange(num_node), np.concatenate([old, new]))
    assert (got[rest] == table[rest]).all()
