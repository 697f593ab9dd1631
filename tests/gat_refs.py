"""Float64 reference, measured error bounds and seed-only inputs for the GAT attention kernels
(csrc/gat_attention.hip; fgnn_hip/nn.py gat_attention; examples/models.py GATConv / FusedGATConv).  Plain helper module
shared by tests/test_gat_references.py (CPU: reference and bounds are sound) and tests/test_gat_gpu.py (GPU: the kernels
are held to them).  Everything here runs on the CPU; nothing imports the kernel library or examples/models.py.

Tolerances (DESIGN.md 4.5's procedure, `measured`): for alpha, out, gfeat, gel and ger the bound is
    4 x max |torch fp32 formulation - gat_ref| over the tensor  +  2^-22 |ref|
on the same inputs.  Over the tensor, not row-wise, for all five: alpha lies in [0, 1] and every out row is a convex
combination of N(0, 1) feature rows, so the tensor has ONE scale; a gfeat row, gel and ger are sums of softmax-gradient
terms that cancel (sum_e gs = 0 per destination), so a row's own magnitude or its own fp32 deviation is no scale for
another summation order's error in that row."""
import functools

import numpy as np
import torch

import train_refs as tr

NSRC, NDST = tr.NSRC, tr.NDST
SLOPE = 0.2
HEADS_FEATS = ((1, 1), (3, 7), (8, 32), (1, 64), (4, 33), (8, 64))
STRUCTS = ("gat_sorted", "gat_unsorted", "fused_sorted", "fused_permuted", "e33")
F_PAD, F_OFF, O_PAD, O_OFF = 13, 5, 24, 8  # feat / out and gout / gfeat are column blocks of wider matrices

# the destinations of the block below that the tests look at by name
DST_NONE, DST_ONE, DST_200, DST_HUB = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def gat_block():
    """(row, col, perm) int64 numpy: destination 0 without an edge, 1 with a single edge, 2 with 200 (a segment that
    crosses 32-edge chunks), 3 a hub with 6001, the other 296 share 3000 random edges (some get none); sorted by
    destination, `perm` shuffles it.  E = 9202 + ...: forced odd, so that E H is no multiple of 4 for odd H."""
    rs = np.random.default_rng(2024)
    col = np.concatenate([np.full(1, DST_ONE), np.full(200, DST_200), np.full(6001, DST_HUB),
                          np.sort(rs.integers(4, NDST, 3001))])
    assert col.size % 2 == 1
    row = rs.integers(0, NSRC, col.size)
    return row, col, rs.permutation(col.size)


def structure(name):
    """(row int64, col int64) numpy"""
    if name.startswith("gat"):
        row, col, perm = gat_block()
        return (row, col) if name == "gat_sorted" else (row[perm], col[perm])
    row, col = tr.agg_structure(name)[:2]
    return row.numpy().astype(np.int64), col.numpy().astype(np.int64)


def philox_keep(seed, step, tag, num_edge, num_head, q):
    """bool [E, H]: the keep mask of the kernels -- element e H + h is word (e H + h) % 4 of Philox block (e H + h) // 4
    keyed (seed, step, tag), kept iff the word >= int(float32(q) 2^32)"""
    n = num_edge * num_head
    words = tr.philox_blocks(seed, step, tag, (n + 3) // 4).reshape(-1)[:n]
    return (words >= np.uint32(int(float(np.float32(q)) * 2 ** 32))).reshape(num_edge, num_head)


def keep_scale(keep, q):
    """float64 [E, H]: keep / (1 - q) with the kernels' fp32 scale"""
    return keep.astype(np.float64) * float(tr.dropout_scale(q))


def gat_ref(row, col, feat, el, er, num_dst, slope=SLOPE, out0=None, ks=None, gout=None, dtype=np.float64):
    """The reference, an explicit loop over the destinations in `dtype` (float64; float32 gives an honest fp32
    formulation with a third summation order).  Returns a dict: alpha [E, H], out [num_dst, H, F] (out0 + the sums) and,
    with gout, gfeat [num_src, H, F], gel [num_src, H], ger [num_dst, H].  ks [E, H]: keep / (1 - q), None = ones."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    feat, el, er = (np.asarray(t, dtype=dtype) for t in (feat, el, er))
    E, (num_src, H, F) = row.size, feat.shape
    slope = dtype(slope)
    ks = np.ones((E, H), dtype=dtype) if ks is None else np.asarray(ks, dtype=dtype)
    alpha = np.zeros((E, H), dtype=dtype)
    out = np.zeros((num_dst, H, F), dtype=dtype) if out0 is None else np.array(out0, dtype=dtype)
    res = dict(alpha=alpha, out=out)
    if gout is not None:
        gout = np.asarray(gout, dtype=dtype)
        res.update(gfeat=np.zeros((num_src, H, F), dtype=dtype), gel=np.zeros((num_src, H), dtype=dtype),
                   ger=np.zeros((num_dst, H), dtype=dtype))
    order = np.argsort(col, kind="stable")
    bounds = np.searchsorted(col[order], np.arange(num_dst + 1))
    for v in range(num_dst):
        idx = order[bounds[v]:bounds[v + 1]]
        if idx.size == 0:
            continue
        x = el[row[idx]] + er[v]
        s = np.where(x > 0, x, slope * x)
        p = np.exp(s - s.max(axis=0))
        a = p / p.sum(axis=0)
        alpha[idx] = a
        at = a * ks[idx]
        fr = feat[row[idx]]
        out[v] += (at[:, :, None] * fr).sum(axis=0)
        if gout is not None:
            g = gout[v]
            ga = (fr * g).sum(axis=-1) * ks[idx]
            gs = a * (ga - (a * ga).sum(axis=0))
            gpre = gs * np.where(x > 0, dtype(1), slope)
            np.add.at(res["gfeat"], row[idx], at[:, :, None] * g)
            np.add.at(res["gel"], row[idx], gpre)
            res["ger"][v] += gpre.sum(axis=0)
    return res


def gat_torch(row, col, feat, el, er, num_dst, slope=SLOPE, out0=None, ks=None, gout=None, dtype=torch.float32):
    """the op-by-op torch formulation on the CPU in `dtype` under autograd (gather, scatter amax, index_add_): what a
    user without the kernels would write, and the yardstick of the measured bounds"""
    row, col = torch.as_tensor(row).long(), torch.as_tensor(col).long()
    feat, el, er = (torch.as_tensor(np.asarray(t)).to(dtype).clone().requires_grad_() for t in (feat, el, er))
    H = feat.shape[1]
    e = torch.nn.functional.leaky_relu(el[row] + er[col], slope)
    m = torch.full((num_dst, H), float("-inf"), dtype=dtype)
    m = m.scatter_reduce(0, col.unsqueeze(1).expand_as(e), e.detach(), reduce="amax", include_self=True)
    p = torch.exp(e - m[col])
    z = torch.zeros((num_dst, H), dtype=dtype).index_add_(0, col, p)
    a = p / z[col]
    at = a if ks is None else a * torch.as_tensor(np.asarray(ks)).to(dtype)
    out = torch.zeros((num_dst,) + tuple(feat.shape[1:]), dtype=dtype) if out0 is None else \
        torch.as_tensor(np.asarray(out0)).to(dtype).clone()
    out = out.index_add(0, col, feat[row] * at.unsqueeze(-1))
    res = dict(alpha=a.detach().numpy(), out=out.detach().numpy())
    if gout is not None:
        gf, gl, gr = torch.autograd.grad(out, (feat, el, er), torch.as_tensor(np.asarray(gout)).to(dtype))
        res.update(gfeat=gf.numpy(), gel=gl.numpy(), ger=gr.numpy())
    return res


# ---- cases ----------------------------------------------------------------------------------------------------------------
# (structure, H, F, kind): kind 'normal' (el, er ~ N(0, 1)), 'overflow' (el, er uniform in +-50: scores span about
# +-100, exp without the max subtraction overflows), or a dropout probability

def cases():
    out = []
    for i, (H, F) in enumerate(HEADS_FEATS):
        out += [("gat_sorted", H, F, "normal"), ("gat_unsorted", H, F, "normal"),
                (STRUCTS[2 + i % 3], H, F, "normal")]
    out += [("gat_sorted", 8, 32, "overflow"), ("gat_unsorted", 3, 7, "overflow")]
    out += [("gat_unsorted", 3, 7, 0.6), ("gat_unsorted", 3, 7, 0.1), ("gat_sorted", 8, 32, 0.6)]
    return out


def case_id(case):
    return "%s-%dx%d-%s" % case


DROP_SEED, DROP_STEP, DROP_TAG = 0x1234567855AA, 7, 3


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """dict of numpy arrays: row, col (int64), featbig [NSRC, D + 13], el, er, obig [NDST, D + 24] (out0 in columns 8 ..
    8 + D), gbig [NDST, D + 24] (gout likewise), ks (None without dropout)"""
    name, H, F, kind = case
    row, col = structure(name)
    kinds = {"normal": 0, "overflow": 1, 0.6: 2, 0.1: 3}
    rs = np.random.default_rng(100000 * STRUCTS.index(name) + 1000 * H + 10 * F + kinds[kind])
    D = H * F
    f32 = np.float32
    if kind == "overflow":
        el, er = (rs.uniform(-50, 50, (n, H)).astype(f32) for n in (NSRC, NDST))
    else:
        el, er = (rs.standard_normal((n, H)).astype(f32) for n in (NSRC, NDST))
    ks = None
    if isinstance(kind, float):
        ks = keep_scale(philox_keep(DROP_SEED, DROP_STEP, DROP_TAG, row.size, H, kind), kind)
    return dict(row=row, col=col, H=H, F=F, el=el, er=er, ks=ks, q=kind if isinstance(kind, float) else 0.0,
                featbig=rs.standard_normal((NSRC, D + F_PAD)).astype(f32),
                obig=rs.standard_normal((NDST, D + O_PAD)).astype(f32),
                gbig=rs.standard_normal((NDST, D + O_PAD)).astype(f32))


def case_views(inp):
    """(feat [NSRC, H, F], out0 [NDST, H, F], gout [NDST, H, F]) as contiguous numpy copies of the column blocks"""
    H, F = inp["H"], inp["F"]
    D = H * F
    return (np.ascontiguousarray(inp["featbig"][:, F_OFF:F_OFF + D]).reshape(NSRC, H, F),
            np.ascontiguousarray(inp["obig"][:, O_OFF:O_OFF + D]).reshape(NDST, H, F),
            np.ascontiguousarray(inp["gbig"][:, O_OFF:O_OFF + D]).reshape(NDST, H, F))


QUANTITIES = ("alpha", "out", "gfeat", "gel", "ger")


@functools.lru_cache(maxsize=None)
def expectation(case):
    """(ref dict in float64, bound dict, dev dict): dev[q] = max |torch fp32 - ref| over the tensor, bound[q] = 4 dev[q] +
    2^-22 |ref[q]| elementwise (see the module docstring)"""
    inp = case_inputs(case)
    feat, out0, gout = case_views(inp)
    args = (inp["row"], inp["col"], feat, inp["el"], inp["er"], NDST)
    ref = gat_ref(*args, out0=out0, ks=inp["ks"], gout=gout)
    t32 = gat_torch(*args, out0=out0, ks=inp["ks"], gout=gout)
    dev = {q: float(np.abs(t32[q].astype(np.float64) - ref[q]).max()) for q in QUANTITIES}
    bound = {q: 4 * dev[q] + 2.0 ** -22 * np.abs(ref[q]) for q in QUANTITIES}
    return ref, bound, dev


def check(got, case, quantities=QUANTITIES, what=""):
    """asserts every quantity of `got` (dict of arrays) within its bound; returns {quantity: worst ratio}"""
    ref, bound, dev = expectation(case)
    ratios = {}
    for q in quantities:
        print("%s %s %s: torch fp32 deviation %.3g" % (what, case_id(case), q, dev[q]))
        ratios[q] = tr.assert_within(np.asarray(got[q]), ref[q], bound[q], "%s %s %s" % (what, case_id(case), q))
    return ratios
