"""Float64 references, derived error bounds and seed-only input generators for the training-side kernels
(csrc/block_aggregate.hip, csrc/gnn_layers.hip, csrc/train_ops.hip; fgnn_hip/nn.py).  Plain helper module, shared by
tests/test_train_kernel_references.py (CPU: the references and bounds are sound) and
tests/test_train_kernel_references_gpu.py (GPU: the kernels are held to them).  Everything here runs on the CPU in
numpy / torch float64; nothing imports the kernel library.

Two kinds of tolerance:
  derived   aggregation and weighted degrees: a bound from the rounding model of an fp32 sum (below), no atol
  measured  softmax_xent, Adam, relu_l2norm: a multiple of the deviation of torch's own fp32 formulation from the
            float64 reference on the same inputs (computed here, on the CPU), plus a few ulp of the reference"""
import functools

import numpy as np
import torch

NSRC, NDST = 2000, 300
U23 = 2.0 ** -23


# ---- comparison ---------------------------------------------------------------------------------------------------------

def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (elements with bound == 0 must be equal: they count as 0 or inf)"""
    got, ref, bound = (torch.as_tensor(t).detach().cpu().double() for t in (got, ref, bound))
    bound = bound.expand_as(ref)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                             torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_within(got, ref, bound, what):
    """prints the worst error / bound ratio before asserting it is <= 1"""
    r = worst_ratio(got, ref, bound)
    print("%s: worst |got - ref| / bound = %.4g" % (what, r))
    assert r <= 1.0, "%s: |got - ref| exceeds its bound %.4g-fold" % (what, r)
    return r


# ---- Philox and dropout --------------------------------------------------------------------------------------------------

def philox_blocks(seed, step, tag, n4, first=0):
    """uint32[n4, 4]: Philox4x32-10 blocks t = first .. first + n4 - 1 addressed as csrc/fgnn_device.h:philox_block is
    by relu_dropout_kernel: counter (block = t >> 32, item = lo32(t), tag, lo32(step)), key (lo32(seed), hi32(seed) ^
    hi32(step))"""
    m32 = np.uint64(0xFFFFFFFF)
    t = np.arange(n4, dtype=np.uint64) + np.uint64(first)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    c0, c1 = t >> np.uint64(32), t & m32
    c2 = np.full(n4, int(tag) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(n4, step & 0xFFFFFFFF, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) ^ (step >> 32)) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2  # 32 x 32 -> 64 bits: no overflow
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & m32, n2, p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def dropout_scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def dropout_ref(x, p, seed, step, tag):
    """relu + dropout of fgnn_relu_dropout, to be compared for equality: element i uses word i % 4 of block i // 4, is
    kept iff the word >= int(float32(p) * 2^32) (every element when p <= 0); kept positive elements are multiplied by
    1 / (1 - p) in fp32, everything else is +0"""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    flat = x.reshape(-1)
    assert flat.size % 4 == 0
    if p <= 0:
        keep = np.ones(flat.size, dtype=bool)
    else:
        thr = int(float(np.float32(p)) * 2 ** 32)
        keep = philox_blocks(seed, step, tag, flat.size // 4).reshape(-1) >= np.uint32(thr)
    y = np.where((flat > 0) & keep, flat * dropout_scale(p), np.float32(0)).astype(np.float32)
    return y.reshape(x.shape)


# ---- aggregation ----------------------------------------------------------------------------------------------------------

def degree_factor(deg, mode, dtype=torch.float64):
    """the layers' degree scalings of max(deg, 1): 0 none, 1 d^-1/2, 2 1 / d"""
    d = torch.as_tensor(deg).to(dtype).clamp(min=1)
    return torch.ones_like(d) if mode == 0 else (d.pow(-0.5) if mode == 1 else 1.0 / d)


def _aggregate(row, col, w, h, num_dst, src_deg, src_mode, dst_deg, dst_mode, out0, dtype):
    row, col = torch.as_tensor(row).long(), torch.as_tensor(col).long()
    h = torch.as_tensor(h).to(dtype)
    ew = torch.ones(row.numel(), dtype=dtype) if w is None else torch.as_tensor(w).to(dtype)
    if src_mode:
        ew = ew * degree_factor(src_deg, src_mode, dtype)[row]
    terms = ew.unsqueeze(1) * h[row]
    fd = degree_factor(dst_deg, dst_mode, dtype).unsqueeze(1) if dst_mode else torch.ones((num_dst, 1), dtype=dtype)
    out0 = torch.zeros((num_dst, h.shape[1]), dtype=dtype) if out0 is None else torch.as_tensor(out0).to(dtype)
    zero = torch.zeros((num_dst, h.shape[1]), dtype=dtype)
    return out0, fd, zero.clone().index_add_(0, col, terms), zero.index_add_(0, col, terms.abs())


def aggregate_ref(row, col, w, h, num_dst, src_deg=None, src_mode=0, dst_deg=None, dst_mode=0, out0=None):
    """(ref, S, k) in float64: ref = out0 + f_dst * sum_e w_e f_src h[row_e] over the edges with col_e = the row,
    S = |out0| + f_dst * sum_e |w_e f_src h[row_e]| per output element, k = the edge count of every destination"""
    out0, fd, s, s_abs = _aggregate(row, col, w, h, num_dst, src_deg, src_mode, dst_deg, dst_mode, out0, torch.float64)
    k = torch.bincount(torch.as_tensor(col).long(), minlength=num_dst)
    return out0 + fd * s, out0.abs() + fd * s_abs, k


def aggregate_fp32(row, col, w, h, num_dst, src_deg=None, src_mode=0, dst_deg=None, dst_mode=0, out0=None):
    """the honest fp32 formulation on the CPU: index_add_ of the fp32 products, times the fp32 factor, onto out0"""
    out0, fd, s, _ = _aggregate(row, col, w, h, num_dst, src_deg, src_mode, dst_deg, dst_mode, out0, torch.float32)
    return out0 + fd * s


def aggregate_bound(S, k, extra=8):
    """|got - ref| <= (k + extra) 2^-23 S.  A sum of k fp32 terms in ANY order (out0 and the partial sums of the
    waves included: a run of k edges cut into m chunks is k - m additions in registers and m atomic additions) carries
    at most (k - 1) u of the terms' magnitudes, u = 2^-24; the products w f_src, (w f_src) h, f_dst acc and the two
    factors' own roundings add a handful of u more (extra = 8 covers them).  2^-23 instead of 2^-24: rsqrt and the
    reciprocal are hardware approximations whose ulp error is not documented.  No atol."""
    return (k.double().unsqueeze(1) + extra) * U23 * S


def degrees_ref(col, w, num_dst):
    """(sum of w per destination in float64, sum of |w|, edge count)"""
    col = torch.as_tensor(col).long()
    w = torch.as_tensor(w).double()
    z = torch.zeros(num_dst, dtype=torch.float64)
    return z.clone().index_add_(0, col, w), z.index_add_(0, col, w.abs()), torch.bincount(col, minlength=num_dst)


def degrees_bound(s_abs, k):
    """|got - ref| <= (k + 2) 2^-23 sum|w|: the same rounding model, a sum of k terms without products"""
    return (k.double() + 2) * U23 * s_abs


AGG_DIMS = (1, 63, 64, 65, 128, 129, 256, 257, 600)
AGG_STRUCTS = ("e1", "e31", "e32", "e33", "one_dst", "e127", "e128", "e129", "fused_sorted", "own_dst", "fused_permuted")
DEGREE_STRUCTS = AGG_STRUCTS + ("runs",)
SCALED_MODES = ((0, 0), (1, 1), (0, 2), (2, 0), (2, 1))


def _fused_block():
    """row, col, permutation of the 6001-edge block of tests/test_fused_gnn_gpu.py (a hub destination whose run crosses
    a workgroup boundary, destinations and sources without an edge, a hub source)"""
    import test_fused_gnn_gpu as f
    assert (f.E, f.NSRC, f.NDST) == (6001, NSRC, NDST)
    row, col, _, perm = f._make_edges()
    return row.numpy(), col.numpy(), perm.numpy()


@functools.lru_cache(maxsize=None)
def agg_structure(name):
    """(row int32, col int32, w fp32, src_deg fp32, dst_deg fp32) as CPU tensors, a function of the name only.
    w: non-integer values in (0, 1.5), the edges of every fifth destination scaled down so that its weight sum is below
    1 (the max(d, 1) clamp on a non-zero degree); dst_deg: the weight sums (PinSAGE's); src_deg: the edge counts with
    every seventh source forced to 0 and every eleventh off the integers -- REFERENCED sources with degree 0 and with a
    non-integer degree.  'runs': for the run-head ballots -- a run of exactly 32 edges that fills the second 32-edge
    chunk, one that starts on the last lane of the first chunk, one that fills a 64-edge wave of the degree kernel"""
    rs = np.random.default_rng(1000 + DEGREE_STRUCTS.index(name))
    if name.startswith("fused"):
        row, col, perm = _fused_block()
        if name == "fused_permuted":
            row, col = row[perm], col[perm]
    elif name == "one_dst":  # one destination owns every edge: the run crosses waves and workgroups, one output row
        row, col = rs.integers(0, NSRC, 4099), np.full(4099, 137)
    elif name == "own_dst":  # every edge a destination of its own, sorted
        row, col = rs.integers(0, NSRC, NDST), np.arange(NDST)
    elif name == "runs":
        col = np.concatenate([np.arange(31), np.full(10, 50), 51 + np.arange(23),  # edges 0-30 | 31-40 | 41-63
                              np.full(32, 200), 201 + np.arange(32),                # 64-95 (a whole chunk) | 96-127
                              np.full(64, 250), np.full(5, 251)])                   # 128-191 (a whole wave) | 192-196
        row = rs.integers(0, NSRC, col.size)
    else:
        e = int(name[1:])
        row, col = rs.integers(0, NSRC, e), np.sort(rs.integers(0, NDST, e))
    w = (0.001 + 1.498 * rs.random(col.size)).astype(np.float32)
    w[col % 5 == 0] *= np.float32(0.02)
    assert (w > 0).all() and (w < 1.5).all()
    dst_deg = np.bincount(col, weights=w.astype(np.float64), minlength=NDST).astype(np.float32)
    src_deg = np.bincount(row, minlength=NSRC).astype(np.float32)
    src_deg[::7] = 0
    src_deg[::11] += np.float32(0.37)
    t = torch.from_numpy
    return (t(row.astype(np.int32)), t(col.astype(np.int32)), t(w), t(src_deg), t(dst_deg))


def agg_pairs():
    """(structure, dim): every structure with two dims, every dim with at least two structures, the two largest
    structures also at the dims that take the masked last trip of the four-column kernel"""
    pairs = []
    for s, name in enumerate(AGG_STRUCTS):
        pairs += [(name, AGG_DIMS[(2 * s) % 9]), (name, AGG_DIMS[(2 * s + 1) % 9])]
    return pairs + [("fused_permuted", 600), ("one_dst", 257)]


def agg_cases():
    """(structure, dim, kernel, (src_mode, dst_mode), weighted): each pair once through fgnn_block_aggregate_ex and once
    through fgnn_block_aggregate_scaled (the five mode pairs in turn); fused_sorted x 257 with all five"""
    cases = []
    for i, (name, dim) in enumerate(agg_pairs()):
        cases.append((name, dim, "ex", (0, 0), i % 2 == 1))
        cases.append((name, dim, "scaled", SCALED_MODES[i % 5], True))
    cases += [("fused_sorted", 257, "scaled", m, True) for m in SCALED_MODES if ("fused_sorted", 257, "scaled", m, True)
              not in cases]
    cases.append(("fused_sorted", 129, "scaled", (1, 1), False))
    return cases


def case_id(case):
    name, dim, kernel, modes, weighted = case
    return "%s-%d-%s-%d%d-%s" % (name, dim, kernel, modes[0], modes[1], "w" if weighted else "1")


H_PAD, H_OFF, O_PAD, O_OFF = 13, 5, 24, 8


@functools.lru_cache(maxsize=4)
def agg_tensors(name, dim):
    """(hbig fp32 [NSRC, dim + 13], obig fp32 [NDST, dim + 24]): h is columns 5 .. 5 + dim of hbig, the output block
    columns 8 .. 8 + dim of obig, which enters holding random non-zero values"""
    g = torch.Generator().manual_seed(7919 * AGG_STRUCTS.index(name) + dim)
    return (torch.randn((NSRC, dim + H_PAD), generator=g), torch.randn((NDST, dim + O_PAD), generator=g))


def agg_case_inputs(case):
    """the arguments of aggregate_ref / aggregate_fp32 for a case (CPU tensors)"""
    name, dim, kernel, (src_mode, dst_mode), weighted = case
    row, col, w, src_deg, dst_deg = agg_structure(name)
    hbig, obig = agg_tensors(name, dim)
    return dict(row=row, col=col, w=w if weighted else None, h=hbig[:, H_OFF:H_OFF + dim], num_dst=NDST,
                src_deg=src_deg if src_mode else None, src_mode=src_mode, dst_deg=dst_deg if dst_mode else None,
                dst_mode=dst_mode, out0=obig[:, O_OFF:O_OFF + dim])


BACKWARD_DIMS = (65, 257, 600)


def backward_inputs(dim):
    """(row, col, w, h fp32 [NSRC, dim], gout fp32 [NDST, dim]) on the fused block"""
    row, col, w, _, _ = agg_structure("fused_sorted")
    g = torch.Generator().manual_seed(31 + dim)
    return row, col, w, torch.randn((NSRC, dim), generator=g), torch.randn((NDST, dim), generator=g)


# ---- bit-exact aggregation on single-flush blocks ------------------------------------------------------------------------
# A block in which every destination owns ONE run of edges and no run crosses a multiple of 32 in the edge array (the
# kernel's chunk per wave): every output element then receives exactly one atomic add, so the result does not depend on
# any order between waves and equals a sequential fp32 computation.  The derived bound above cannot tell a reordered
# accumulation inside a wave from the original; equality with sequential_f32 can.

EXACT_DIMS = (1, 64, 65, 128, 129, 257, 600)
EXACT_NSRC, EXACT_NDST = 40, 40
EXACT_CHUNK = 32
# chunk by chunk: one run of 32, (k, 32 - k) for k = 1 .. 15, (16, 16), and a last chunk of 13 edges (not a multiple of
# the edge loop's unroll of 4, so its last trip runs on clamped lanes)
EXACT_RUNS = (32,) + tuple(n for k in range(1, 16) for n in (k, 32 - k)) + (16, 16) + (5, 1, 7)


@functools.lru_cache(maxsize=None)
def single_flush_block():
    """(row int32 [E], col int32 [E], w fp32 [E]) as CPU tensors: runs of EXACT_RUNS edges, each to a destination of its
    own (36 of the 40, in scattered order), sources drawn from all 40, non-integer weights in [0.25, 1.5)"""
    rs = np.random.default_rng(4242)
    dst = rs.permutation(EXACT_NDST)[:len(EXACT_RUNS)]
    col = np.repeat(dst, EXACT_RUNS)
    row = rs.integers(0, EXACT_NSRC, col.size)
    w = (0.25 + 1.25 * rs.random(col.size)).astype(np.float32)
    t = torch.from_numpy
    return t(row.astype(np.int32)), t(col.astype(np.int32)), t(w)


@functools.lru_cache(maxsize=None)
def exact_tensors(dim):
    """(hbig fp32 [40, dim + 13], obig fp32 [40, dim + 24]) with h = columns 5 .. 5 + dim and the output block = columns
    8 .. 8 + dim (H_OFF, O_OFF); magnitudes in [0.25, 2) with random signs: no product or sum comes near a denormal"""
    rs = np.random.default_rng(9000 + dim)

    def draw(shape):
        return ((0.25 + 1.75 * rs.random(shape)) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)
    return torch.from_numpy(draw((EXACT_NSRC, dim + H_PAD))), torch.from_numpy(draw((EXACT_NDST, dim + O_PAD)))


def sequential_f32(row, col, w, h, out0):
    """fp32 [num_dst, dim] (numpy): acc = 0; for each edge in order acc = f32(acc + f32(w * h)); out = f32(out0 + acc),
    every operation rounded to fp32 on its own (no fused multiply-add).  w None: weight 1, out0 None: zeros."""
    row, col, h = np.asarray(row), np.asarray(col), np.asarray(h, dtype=np.float32)
    acc = np.zeros((EXACT_NDST, h.shape[1]), dtype=np.float32)
    for e in range(row.size):
        term = h[row[e]] if w is None else np.float32(w[e]) * h[row[e]]
        acc[col[e]] = acc[col[e]] + term
    assert acc.dtype == np.float32
    return acc if out0 is None else np.asarray(out0, dtype=np.float32) + acc


# ---- softmax cross entropy -----------------------------------------------------------------------------------------------

XENT_C =(1, 2, 64, 65, 255, 256, 257, 1000)
XENT_N = (1, 5, 2500)


@functools.lru_cache(maxsize=None)
def xent_inputs(c, n):
    """(logits fp32 [n, c], labels int64 [n]), a function of (c, n).  Rows by index % 8: 1 all equal, 2 one +80 among
    -80s AT the label, 3 the same OFF the label, 4 a -inf at a class that is not the label, others N(0, 3).  Labels
    include 0 and c - 1; rows 3, 10, 17, ... carry -100, row 4 (n = 5) / row 12 (n = 2500) carries the label c."""
    rs = np.random.default_rng(100000 * c + n)
    x = (3.0 * rs.standard_normal((n, c))).astype(np.float32)
    y = rs.integers(0, c, n).astype(np.int64)
    y[0] = 0
    if n > 1:
        y[1] = c - 1
    for i in range(n):
        kind, lab = i % 8, int(y[i])
        other = (lab + 1 + int(rs.integers(0, max(c - 1, 1)))) % c  # != lab when c > 1
        if kind == 1:
            x[i] = np.float32(1.25)
        elif kind == 2 or (kind == 3 and c > 1):
            x[i] = -80.0
            x[i, lab if kind == 2 else other] = 80.0
        elif kind == 4 and c > 1:
            x[i, other] = -np.inf
    y[3::7] = -100
    if n > 4:
        y[4 if n == 5 else 12] = c
    return torch.from_numpy(x), torch.from_numpy(y)


def xent_ref(logits, labels):
    """(loss, grad) in float64: the mean of lse(x_i) - x_i[y_i] over the rows whose label lies in [0, C) and its
    gradient; every other row has a zero gradient row"""
    x = torch.as_tensor(logits).double()
    y = torch.as_tensor(labels).long()
    n, c = x.shape
    valid = (y >= 0) & (y < c)
    nv = max(int(valid.sum()), 1)
    m = x.max(dim=1, keepdim=True)[0]
    e = torch.exp(x - m)
    s = e.sum(dim=1, keepdim=True)
    lse = (m + torch.log(s)).squeeze(1)
    ys = torch.where(valid, y, torch.zeros_like(y))
    row_loss = lse - x.gather(1, ys.unsqueeze(1)).squeeze(1)
    loss = torch.where(valid, row_loss, torch.zeros_like(row_loss)).sum() / nv
    grad = e / s
    grad[torch.arange(n), ys] -= 1.0
    grad = torch.where(valid.unsqueeze(1), grad / nv, torch.zeros_like(grad))
    return loss, grad


def xent_torch(logits, labels, dtype):
    """torch.nn.functional.cross_entropy and its gradient on the CPU in `dtype`; labels outside [0, C) are mapped to
    torch's ignore_index first (torch refuses them, the kernel and xent_ref ignore such rows)"""
    x = torch.as_tensor(logits).to(dtype).clone().requires_grad_()
    y = torch.as_tensor(labels).long()
    y = torch.where((y >= 0) & (y < x.shape[1]), y, torch.full_like(y, -100))
    loss = torch.nn.functional.cross_entropy(x, y)
    (grad,) = torch.autograd.grad(loss, x)
    return loss.detach(), grad


def xent_fp32_one_pass(logits, labels):
    """(loss, grad): the one-pass formulation of softmax_xent_kernel in honest fp32 on the CPU -- e = exp(x - max), grad =
    (e * (1 / sum e) - onehot) * (1 / n_valid), loss = sum(lse - x[label]) * (1 / n_valid).  For the CPU test of the
    measured bound only: a second correct fp32 formulation must pass what torch's own sets"""
    x = torch.as_tensor(logits).float()
    y = torch.as_tensor(labels).long()
    n, c = x.shape
    valid = (y >= 0) & (y < c)
    inv_n = torch.tensor(1.0) / torch.tensor(float(max(int(valid.sum()), 1)))
    ys = torch.where(valid, y, torch.zeros_like(y))
    m = x.max(dim=1, keepdim=True)[0]
    e = torch.exp(x - m)
    s = e.sum(dim=1, keepdim=True)
    row_loss = (m + torch.log(s)).squeeze(1) - x.gather(1, ys.unsqueeze(1)).squeeze(1)
    onehot = torch.zeros_like(x).scatter_(1, ys.unsqueeze(1), 1.0)
    grad = torch.where(valid.unsqueeze(1), (e * (1.0 / s) - onehot) * inv_n, torch.zeros_like(x))
    return torch.where(valid, row_loss, torch.zeros_like(row_loss)).sum() * inv_n, grad


@functools.lru_cache(maxsize=None)
def xent_expectation(c, n):
    """(ref loss, ref grad, loss bound, grad bound, d_loss, d_grad [n]): the bounds |loss - ref| <= 4 d_loss + 2^-22
    |ref| and |grad - ref| <= 4 max(d_grad) + 2^-24 / n_valid, d_loss and the per-row d_grad = the deviation of torch's
    fp32 cross_entropy (CPU) from xent_ref.  max(d_grad) runs over the rows: a row's own deviation is no scale for
    another formulation's error in that row -- in some of 2500 rows torch lands within a tenth of an ulp, and 2^-24 /
    n_valid alone is one ulp of a gradient entry near 1 / n_valid, less than expf's own error (xent_fp32_one_pass
    exceeds such a per-row bound on the CPU; it passes this one)"""
    x, y = xent_inputs(c, n)
    loss, grad = xent_ref(x, y)
    loss32, grad32 = xent_torch(x, y, torch.float32)
    nv = max(int(((y >= 0) & (y < c)).sum()), 1)
    d_loss = (loss32.double() - loss).abs()
    d_grad = (grad32.double() - grad).abs().max(dim=1)[0]
    return (loss, grad, 4 * d_loss + 2.0 ** -22 * loss.abs(), 4 * d_grad.max() + 2.0 ** -24 / nv, d_loss, d_grad)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------

def f32(v):
    return float(np.float32(v))


ADAM = dict(lr=f32(0.1), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8))
ADAM_WD = (0.0, f32(0.01))
ADAM_STEPS = 4
ADAM_SETS = ("eight", "nine", "seventeen", "stride", "largest_last")


def adam_shapes(name, cus):
    """no tensor (but the empty one) has fewer than 33 elements: the tolerance is a multiple of the LARGEST deviation of
    torch's fp32 update over the tensor, and over one or six elements that maximum can be no deviation at all -- the
    bound would then be 2^-24 max|ref|, half an ulp, which no fp32 computation of several steps meets"""
    small = [(33,), (7, 5), (64,), (41,), (129,), (300,), (12, 3), (257,)]
    return {"eight": small, "nine": small + [(40,)], "seventeen": small + small + [(1029,)],
            "stride": [(8 * cus * 256 + 77,)],  # a second trip of the kernel's stride loop (at most 8 x CUs workgroups)
            "largest_last": [(37,), (300,), (4099,)],
            "zero_length": [(40,), (0,), (300,)]}[name]


def adam_grads(name, cus):
    """[step][tensor] fp32 N(0, 1)"""
    g = torch.Generator().manual_seed(17 + sum(map(ord, name)))
    return [[torch.randn(s, generator=g) for s in adam_shapes(name, cus)] for _ in range(ADAM_STEPS)]


def adam_ref(grads, lr, betas, eps, weight_decay):
    """[step][tensor] float64 parameters after each step, from zero: torch's documented Adam (no amsgrad, L2 weight decay
    folded into the gradient), the bias corrections in float64 like everything else"""
    b1, b2 = betas
    p = [torch.zeros(g.shape, dtype=torch.float64) for g in grads[0]]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    out = []
    for t, gs in enumerate(grads, start=1):
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        for k, g in enumerate(gs):
            g = g.double() + weight_decay * p[k]
            m[k] = b1 * m[k] + (1.0 - b1) * g
            v[k] = b2 * v[k] + (1.0 - b2) * g * g
            p[k] = p[k] - (lr / bc1) * m[k] / (v[k].sqrt() / bc2 ** 0.5 + eps)
        out.append([t_.clone() for t_ in p])
    return out


def adam_torch(grads, lr, betas, eps, weight_decay, dtype):
    """[step][tensor]: torch.optim.Adam on the CPU in `dtype`, from zero"""
    ps = [torch.zeros(g.shape, dtype=dtype).requires_grad_() for g in grads[0]]
    live = [p for p in ps if p.numel()]
    opt = torch.optim.Adam(live, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(dtype).clone()
        opt.step()
        out.append([p.detach().clone() for p in ps])
    return out


def adam_expectation(name, cus, wd):
    """(grads, [step][tensor] ref, [step][tensor] bound, [step][tensor] dev): dev = max|torch fp32 - ref| of the tensor,
    bound = 4 dev + 2^-24 max|ref|"""
    grads = adam_grads(name, cus)
    ref = adam_ref(grads, weight_decay=wd, **ADAM)
    t32 = adam_torch(grads, weight_decay=wd, dtype=torch.float32, **ADAM)
    dev = [[float((a.double() - r).abs().max()) if r.numel() else 0.0 for a, r in zip(a_s, r_s)]
           for a_s, r_s in zip(t32, ref)]
    bound = [[torch.tensor(4 * d + 2.0 ** -24 * (float(r.abs().max()) if r.numel() else 0.0)) for d, r in zip(d_s, r_s)]
             for d_s, r_s in zip(dev, ref)]
    return grads, ref, bound, dev


# ---- relu + row L2 norm -------------------------------------------------------------------------------------------------------

L2_DIMS = (7, 300)
X_PAD, X_OFF, G_PAD, G_OFF = 9, 3, 6, 2


def l2norm_rows(cus):
    return 8 * cus * 4 + 5  # a second trip of the row loop (at most 8 x CUs workgroups of 4 waves)


@functools.lru_cache(maxsize=2)
def l2norm_inputs(dim, rows):
    """(xbig fp32 [rows, dim + 9], gbig fp32 [rows, dim + 6]): x = columns 3 .. 3 + dim, gout = columns 2 .. 2 + dim;
    |x| >= 0.25 (the gradient's conditioning is 1 / norm), every tenth row without a positive entry"""
    g = torch.Generator().manual_seed(500 + dim)
    xbig = torch.randn((rows, dim + X_PAD), generator=g)
    xbig = xbig + 0.25 * torch.sign(xbig)
    xbig[::10] = -xbig[::10].abs()
    return xbig, torch.randn((rows, dim + G_PAD), generator=g)


def relu_l2norm_ref(x, gout, dtype=torch.float64):
    """(y, inv_norm, gx) in `dtype`: z = relu(x), y = z / where(|z| == 0, 1, |z|); gx = (gout - y <gout, y>) / |z| where
    x > 0, else 0 (a row without a positive entry: y = 0, inv_norm = 1, gx = 0)"""
    x, gout = torch.as_tensor(x).to(dtype), torch.as_tensor(gout).to(dtype)
    z = torch.relu(x)
    n = z.pow(2).sum(dim=1, keepdim=True).sqrt()
    inv = 1.0 / torch.where(n == 0, torch.ones_like(n), n)
    y = z * inv
    gx = torch.where(x > 0, (gout - y * (gout * y).sum(dim=1, keepdim=True)) * inv, torch.zeros_like(x))
    return y, inv.squeeze(1), gx


def relu_l2norm_torch(x, gout):
    """(y, gx): the op-by-op torch formulation in fp32 under autograd on the CPU (the one the fused layer replaced)"""
    x = torch.as_tensor(x).float().clone().requires_grad_()
    z = torch.relu(x)
    n = z.norm(2, 1, keepdim=True)
    y = z / torch.where(n == 0, torch.ones_like(n), n)
    (gx,) = torch.autograd.grad(y, x, torch.as_tensor(gout).float())
    return y.detach(), gx


def l2norm_expectation(dim, rows):
    """(y, inv, gx references; y bound, gx bound; d_y, d_gx per row): bound = 4 x the deviation of the torch fp32
    formulation from the reference + 2^-22 |ref|.  Forward: the row's largest deviation.  Backward: the largest
    deviation of the whole tensor -- a row's own deviation says nothing about another formulation's error there: in a
    row with ONE positive entry the true gradient is 0, torch gets y = z / n = 1 and so exactly 0, while y = z * (1 /
    n) can be 1 - 2^-24 and leaves 2^-24 |gout| behind (tests/test_train_kernel_references.py runs that formulation in
    fp32 on the CPU against this bound)."""
    xbig, gbig = l2norm_inputs(dim, rows)
    x, gout = xbig[:, X_OFF:X_OFF + dim], gbig[:, G_OFF:G_OFF + dim]
    y, inv, gx = relu_l2norm_ref(x, gout)
    y32, gx32 = relu_l2norm_torch(x, gout)
    d_y = (y32.double() - y).abs().max(dim=1, keepdim=True)[0]
    d_gx = (gx32.double() - gx).abs().max(dim=1, keepdim=True)[0]
    return y, inv, gx, 4 * d_y + 2.0 ** -22 * y.abs(), 4 * d_gx.max() + 2.0 ** -22 * gx.abs(), d_y, d_gx


# ---- dynamic cache table ---------------------------------------------------------------------------------------------------------

EMPTY = 0xFFFFFFFF
# (table entries, old nodes, new nodes, old ids distinct).  A table of 50 000 entries cannot hold 70 001 DISTINCT ids:
# the 70 001-entry old list on it repeats ids (every copy writes EMPTY: still deterministic), and the case with 70 001
# distinct old and new ids runs on a table of 100 000 entries
CACHE_CASES = ((50000, 0, 4000, True), (50000, 4000, 0, True), (50000, 1, 1, True), (50000, 0, 1, True),
               (50000, 1, 0, True), (50000, 20011, 17003, True), (50000, 70001, 30001, False),
               (100000, 70001, 70001, True))


def cache_replace_inputs(num_node, n_old, n_new, distinct):
    """(rank uint32 [num_node], num_cached, old uint32, new uint32); the lists overlap in part (distinct ids each,
    except an old list longer than the table)"""
    rs = np.random.default_rng(num_node + 3 * n_old + 7 * n_new)
    rank = rs.permutation(num_node).astype(np.uint32)
    num_cached = num_node // 4
    perm = rs.permutation(num_node).astype(np.uint32)
    at = int(np.nonzero(perm == rank[0])[0][0])  # the first old node is a cached one: even a list of one changes the table
    perm[0], perm[at] = perm[at], perm[0]
    old = perm[:n_old] if distinct else rs.integers(0, num_node, n_old).astype(np.uint32)
    shift = max(n_old // 2, 1) if distinct else 0  # half of the old list is in the new one too
    new = np.roll(perm, -shift)[:n_new].copy()
    return rank, num_cached, np.ascontiguousarray(old), new


def cache_replace_ref(table, old, new):
    """ReplaceCacheGPU's index update: old nodes -> EMPTY, then new node i -> i (a node in both ends with its new slot)"""
    t = np.array(table, dtype=np.uint32, copy=True)
    t[old] = EMPTY
    t[new] = np.arange(new.size, dtype=np.uint32)
    return t
