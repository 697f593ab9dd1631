"""Float64 reference of the CSR aggregation (csrc/csr_aggregate.hip; fgnn_hip.nn.csr_aggregate_into) and the synthetic
graph its tests run on.  Plain helper module, shared by tests/test_csr_aggregate_references.py (CPU: the reference is
sound) and tests/test_csr_aggregate_gpu.py (GPU: the kernel is held to it).  numpy only; nothing imports the kernel
library.

For output row i, v = nodes[i] if nodes is given, else first + i, over v's CSR range [indptr[v], indptr[v + 1]):
    out[i, c] = f_dst(v) * sum_p w[p] * f_src(indices[p]) * h[indices[p], c]
f by mode of max(d, 1): 0 -> 1, 1 -> d^-1/2, 2 -> 1 / d; d = src_deg[indices[p]] for f_src, dst_deg[v] for f_dst, or the
row's own length where dst_deg is None.  fp16 input is upcast exactly (every binary16 value is a float64 value)."""
import numpy as np


def degree_factor(deg, mode):
    d = np.maximum(np.asarray(deg, dtype=np.float64), 1.0)
    return np.ones_like(d) if mode == 0 else (d ** -0.5 if mode == 1 else 1.0 / d)


def rows_of(indptr, nodes=None, first=0, count=None):
    """the node ids a call computes, as int64"""
    if nodes is not None:
        return np.asarray(nodes).astype(np.int64)
    n = len(indptr) - 1 - first if count is None else count
    return first + np.arange(n, dtype=np.int64)


def expand(indptr, rows):
    """(pos, dst, k): the CSR positions of the rows' entries, the output row of each, the rows' lengths"""
    indptr = np.asarray(indptr).astype(np.int64)
    beg, k = indptr[rows], indptr[rows + 1] - indptr[rows]
    dst = np.repeat(np.arange(len(rows), dtype=np.int64), k)
    pos = np.arange(int(k.sum()), dtype=np.int64) - np.repeat(np.cumsum(k) - k, k) + np.repeat(beg, k)
    return pos, dst, k


def csr_aggregate_ref(indptr, indices, h, nodes=None, first=0, count=None, w=None, src_deg=None, src_mode=0,
                      dst_deg=None, dst_mode=0):
    """(ref, S, k) in float64: ref as above, S = f_dst * sum_p |w f_src h| per output element (what the rounding bound
    scales with), k = the length of every output row's CSR row"""
    rows = rows_of(indptr, nodes, first, count)
    pos, dst, k = expand(indptr, rows)
    src = np.asarray(indices).astype(np.int64)[pos]
    ew = np.ones(len(pos)) if w is None else np.asarray(w, dtype=np.float64)[pos]
    if src_mode:
        ew = ew * degree_factor(np.asarray(src_deg)[src], src_mode)
    terms = ew[:, None] * np.asarray(h)[src].astype(np.float64)
    dim = terms.shape[1]
    s, s_abs = np.zeros((len(rows), dim)), np.zeros((len(rows), dim))
    nz = k > 0
    if len(pos):  # reduceat over the non-empty rows' starts (consecutive starts of empty rows would repeat entries)
        starts = (np.cumsum(k) - k)[nz]
        s[nz] = np.add.reduceat(terms, starts, axis=0)
        s_abs[nz] = np.add.reduceat(np.abs(terms), starts, axis=0)
    fd = np.ones(len(rows))
    if dst_mode:
        fd = degree_factor(k if dst_deg is None else np.asarray(dst_deg)[rows], dst_mode)
    return fd[:, None] * s, fd[:, None] * s_abs, k


def aggregate_bound(S, k, extra=8):
    """|got - ref| <= (k + extra) 2^-23 S: the bound csrc/block_aggregate.hip documents (tests/train_refs.py,
    aggregate_bound): k fp32 terms summed in any order, a handful of roundings for the products and factors, 2^-23 for
    the hardware rsqrt / reciprocal.  The piece sums of a split row are more additions of the same terms' partial sums:
    k - 1 additions of magnitudes below S in all, as for a sum in one run."""
    return (np.asarray(k, dtype=np.float64)[:, None] + extra) * 2.0 ** -23 * S


# ---- the synthetic graph of tests/test_csr_aggregate_gpu.py ------------------------------------------------------------

NUM_NODE = 120_000
HUB = 100_000
SPECIAL_AT = 1000  # id of the first special row


def special_lengths(split):
    """row lengths from SPECIAL_AT on: empty rows on both sides of the hub and of the longest split row, the small
    lengths around the wave's 32 / 64-entry loads, the lengths around the split"""
    return [0, HUB, 0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, split - 1, split, split + 1, 0, 3 * split + 5, 0]


def synthetic_csr(split, seed=11):
    """(indptr u32 [N + 1], indices u32 [E]): the special rows at SPECIAL_AT .., every other node v with v % 3
    neighbours; a row's neighbours are distinct ids spread over [0, N) (the hub's too), so ids go up to N - 1"""
    rng = np.random.default_rng(seed)
    k = (np.arange(NUM_NODE) % 3).astype(np.int64)
    sp = special_lengths(split)
    k[SPECIAL_AT:SPECIAL_AT + len(sp)] = sp
    indptr = np.zeros(NUM_NODE + 1, dtype=np.int64)
    np.cumsum(k, out=indptr[1:])
    indices = np.empty(indptr[-1], dtype=np.uint32)
    for v in np.flatnonzero(k > 2):  # the special rows: distinct neighbours
        indices[indptr[v]:indptr[v + 1]] = rng.choice(NUM_NODE, size=k[v], replace=False)
    short = np.flatnonzero((k > 0) & (k <= 2))
    pos, _, _ = expand(indptr, short)
    indices[pos] = rng.integers(0, NUM_NODE, size=len(pos))
    indices[indptr[SPECIAL_AT + 1]] = NUM_NODE - 1  # the largest id is read
    return indptr.astype(np.uint32), indices


def special_rows(split):
    """ids of the special rows with one ordinary row on either side"""
    return np.arange(SPECIAL_AT - 1, SPECIAL_AT + len(special_lengths(split)) + 1, dtype=np.int64)
