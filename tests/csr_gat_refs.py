"""Float64 reference, measured bound and seed-only inputs for the GAT attention over whole CSR rows
(csrc/csr_gat_attention.hip; fgnn_hip.nn.csr_gat_attention_into).  Plain helper module shared by
tests/test_csr_gat_references.py (CPU: reference and bound are sound) and tests/test_csr_gat_gpu.py (GPU: the kernel is
held to them).  numpy and torch on the CPU only; nothing imports the kernel library.

For output row i, v = rows[i], over v's CSR range [indptr[v], indptr[v + 1]), H heads of F features:
    s[p, h] = leaky_relu(el[indices[p], h] + er[v, h], slope)      a[p, h] = softmax of s[., h] over the row
    out[i, h, :] = sum_p a[p, h] feat[indices[p], h, :]            (zeros for a row without a neighbour)
The graph is csr_refs.synthetic_csr(split), the rows csr_refs.special_rows(split): lengths 0, 1, 3 .. 5, 31 .. 33,
63 .. 65, split - 1 .. split + 1, 3 split + 5 and 100 000, empty rows on both sides of the hubs.

Tolerance (gat_refs.py, DESIGN.md 4.5: `measured`): 4 x max |torch fp32 formulation - float64 ref| over the tensor +
2^-22 |ref|, the fp32 formulation being gat_refs.gat_torch over the rows' edges expanded to COO on the same inputs.
Over the tensor: every out row is a convex combination of N(0, 1) feature rows, so the tensor has one scale."""
import functools

import numpy as np

import csr_refs
import gat_refs

SLOPE = gat_refs.SLOPE
F_PAD, F_OFF, O_PAD, O_OFF = gat_refs.F_PAD, gat_refs.F_OFF, gat_refs.O_PAD, gat_refs.O_OFF
MAX_DIM = max(H * F for H, F in gat_refs.HEADS_FEATS)


def csr_gat_ref(indptr, indices, feat, el, er, rows, slope=SLOPE):
    """out [len(rows), H, F] in float64: an explicit loop over the rows asked for, head by head (so the 100 000-edge
    hub gathers 100 000 x F values at a time, not 100 000 x H x F)"""
    indptr = np.asarray(indptr).astype(np.int64)
    _, H, F = feat.shape
    out = np.zeros((len(rows), H, F))
    for i, v in enumerate(np.asarray(rows).astype(np.int64)):
        src = np.asarray(indices[indptr[v]:indptr[v + 1]]).astype(np.int64)
        if src.size == 0:
            continue
        for h in range(H):
            x = el[src, h].astype(np.float64) + np.float64(er[v, h])
            s = np.where(x > 0, x, np.float64(slope) * x)
            p = np.exp(s - s.max())
            out[i, h] = (p / p.sum()) @ feat[src, h, :].astype(np.float64)
    return out


def coo_of_rows(indptr, indices, rows):
    """(row, col, srcs): the rows' edges expanded to COO over compact ids -- row indexes `srcs` (the distinct neighbour
    ids, sorted), col the position in `rows`"""
    rows = np.asarray(rows).astype(np.int64)
    pos, col, _ = csr_refs.expand(indptr, rows)
    srcs, row = np.unique(np.asarray(indices)[pos].astype(np.int64), return_inverse=True)
    return row, col, srcs


def csr_gat_torch32(indptr, indices, feat, el, er, rows, slope=SLOPE):
    """the torch fp32 formulation of the same rows: gat_refs.gat_torch over their edges expanded to COO"""
    row, col, srcs = coo_of_rows(indptr, indices, rows)
    rows = np.asarray(rows).astype(np.int64)
    return gat_refs.gat_torch(row, col, np.ascontiguousarray(feat[srcs]), el[srcs], er[rows], len(rows), slope)["out"]


def piecewise_combination(s, feat, split):
    """float64: a row's result from its scores s [k, H] and feature rows [k, H, F], computed piece by piece as the kernel
    defines it -- piece j: m_j, z_j = sum exp(s - m_j), acc_j = sum exp(s - m_j) feat; row: m = max m_j, c_j = exp(m_j -
    m), out = sum c_j acc_j / sum c_j z_j"""
    k = s.shape[0]
    pieces = [(s[a:a + split], feat[a:a + split]) for a in range(0, k, split)]
    ms = [sj.max(axis=0) for sj, _ in pieces]
    m = np.max(ms, axis=0)
    Z = np.zeros(s.shape[1])
    A = np.zeros(feat.shape[1:])
    for (sj, fj), mj in zip(pieces, ms):
        w = np.exp(sj - mj)
        c = np.exp(mj - m)
        Z += c * w.sum(axis=0)
        A += c[:, None] * (w[:, :, None] * fj).sum(axis=0)
    return A / Z[:, None]


# ---- the inputs of tests/test_csr_gat_gpu.py -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def graph(split):
    return csr_refs.synthetic_csr(split)


@functools.lru_cache(maxsize=None)
def feature_matrix():
    """fp32 [NUM_NODE, MAX_DIM + F_PAD]: every case's feat is the column block F_OFF .. F_OFF + H F of it"""
    return np.random.default_rng(3).standard_normal((csr_refs.NUM_NODE, MAX_DIM + F_PAD), dtype=np.float32)


def feat_view(H, F):
    """[NUM_NODE, H, F] view of the case's column block"""
    return feature_matrix()[:, F_OFF:F_OFF + H * F].reshape(csr_refs.NUM_NODE, H, F)


@functools.lru_cache(maxsize=None)
def scores(H, kind):
    """(el, er) fp32 [NUM_NODE, H]: 'normal' N(0, 1), 'overflow' uniform in +-50 (gat_refs' kinds)"""
    rs = np.random.default_rng(1000 * H + (kind == "overflow"))
    if kind == "overflow":
        return tuple(rs.uniform(-50, 50, (csr_refs.NUM_NODE, H)).astype(np.float32) for _ in range(2))
    return tuple(rs.standard_normal((csr_refs.NUM_NODE, H)).astype(np.float32) for _ in range(2))


@functools.lru_cache(maxsize=None)
def expectation(H, F, kind, split):
    """(ref float64 [R, H, F], bound [R, H, F], dev, t32) for the special rows in ascending order: t32 = the torch fp32
    formulation, dev = max |t32 - ref| over the tensor, bound = 4 dev + 2^-22 |ref|.  Measured on the inputs above,
    never on the kernel."""
    indptr, indices = graph(split)
    rows = csr_refs.special_rows(split)
    el, er = scores(H, kind)
    feat = feat_view(H, F)
    ref = csr_gat_ref(indptr, indices, feat, el, er, rows)
    t32 = csr_gat_torch32(indptr, indices, feat, el, er, rows)
    dev = float(np.abs(t32.astype(np.float64) - ref).max())
    return ref, 4 * dev + 2.0 ** -22 * np.abs(ref), dev, t32


def check(got, H, F, kind, split, order=slice(None), what=""):
    """asserts got [R, H, F] (the special rows in `order`) inside the bound; prints the deviation and the worst ratio"""
    ref, bound, dev, _ = expectation(H, F, kind, split)
    what = "%s %dx%d %s" % (what, H, F, kind)
    print("%s: torch fp32 deviation %.3g" % (what, dev))
    return gat_refs.tr.assert_within(np.asarray(got), np.ascontiguousarray(ref[order]),
                                     np.ascontiguousarray(bound[order]), what)
