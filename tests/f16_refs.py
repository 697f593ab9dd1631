"""Float64 numpy reference, shapes and case lists for the half-precision feature path: fp16 rows into the fp32
aggregation kernels (csrc/block_aggregate.hip: fgnn_block_aggregate_ex_f16 / _scaled_f16; csrc/train_ops.hip:
fgnn_sage_finish_z_f16).  Plain helper module shared by tests/test_f16_references.py (CPU: the reference agrees with
train_refs' on the upcast rows) and tests/test_f16_kernels_gpu.py (GPU: the kernels are held to it).  Nothing here
imports the kernel library.

The bound is train_refs.aggregate_bound unchanged, (k + 8) 2^-23 S: binary16 -> binary32 is exact, so the fp16 kernels
add the same fp32 terms as the fp32 kernels fed the upcast rows, and the rounding model of that bound (a sum of k fp32
terms in any order plus a handful of roundings for the products and factors) covers them as it stands."""
import functools

import numpy as np
import torch

import train_refs as R

NSRC, NDST = R.NSRC, R.NDST
DIMS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 256, 257, 600)
# blocks of 1, 31, 32, 33 and 65 edges (sorted destinations), a hub destination of 6001 edges in an unsorted edge
# array, and a block without an edge
HUB_EDGES = 6001
STRUCTS = ("e1", "e31", "e32", "e33", "e65", "hub_unsorted", "empty")
MODE_PAIRS = tuple((s, d) for s in (0, 1, 2) for d in (0, 1, 2))
# (columns left of h, columns right of h) in the wider fp16 matrix the scaled entry point reads h out of: the row
# stride dim + left + right comes out even and odd for every dim, the base 4-byte aligned (even left) or not (odd left)
H_FRAMES = ((4, 6), (4, 7), (3, 8), (5, 4))


def f16_to_f64(h16):
    """binary16 -> float64 through numpy (exact)"""
    a = h16.numpy() if isinstance(h16, torch.Tensor) else np.asarray(h16)
    assert a.dtype == np.float16
    return a.astype(np.float64)


def _factor(deg, mode):
    d = np.maximum(np.asarray(deg, dtype=np.float64), 1.0)
    return np.ones_like(d) if mode == 0 else (d ** -0.5 if mode == 1 else 1.0 / d)


def aggregate_ref_f16(row, col, w, h16, num_dst, src_deg=None, src_mode=0, dst_deg=None, dst_mode=0, out0=None):
    """(ref, S, k) as float64 / int64 numpy arrays: ref = out0 + f_dst sum_e w_e f_src (float64)h16[row_e] over the edges
    with col_e = the row, S = |out0| + f_dst sum_e |w_e f_src h16[row_e]|, k = every destination's edge count"""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    h = f16_to_f64(h16)
    ew = np.ones(row.size) if w is None else np.asarray(w, dtype=np.float64)
    if src_mode:
        ew = ew * _factor(src_deg, src_mode)[row]
    terms = ew[:, None] * h[row]
    s, s_abs = np.zeros((num_dst, h.shape[1])), np.zeros((num_dst, h.shape[1]))
    np.add.at(s, col, terms)
    np.add.at(s_abs, col, np.abs(terms))
    fd = _factor(dst_deg, dst_mode)[:, None] if dst_mode else np.ones((num_dst, 1))
    o = np.zeros_like(s) if out0 is None else np.asarray(out0, dtype=np.float64)
    return o + fd * s, np.abs(o) + fd * s_abs, np.bincount(col, minlength=num_dst)


def bound(S, k):
    """train_refs.aggregate_bound on the numpy triple, as a float64 tensor"""
    return R.aggregate_bound(torch.from_numpy(S), torch.from_numpy(k))


@functools.lru_cache(maxsize=None)
def structure(name):
    """(row int32, col int32, w fp32, src_deg fp32, dst_deg fp32) as CPU tensors, a function of the name only; weights
    and degree vectors drawn the way train_refs.agg_structure draws them (weight sums below 1, referenced sources of
    degree 0 and of non-integer degree)"""
    rs = np.random.default_rng(2600 + STRUCTS.index(name))
    if name == "hub_unsorted":  # destination 137 owns 6001 edges, shuffled among 599 edges of the other destinations
        col = rs.permutation(np.concatenate([np.full(HUB_EDGES, 137), rs.integers(0, NDST, 599)]))
        row = rs.integers(0, NSRC, col.size)
    else:
        e = 0 if name == "empty" else int(name[1:])
        row, col = rs.integers(0, NSRC, e), np.sort(rs.integers(0, NDST, e))
    e = col.size
    w = (0.001 + 1.498 * rs.random(e)).astype(np.float32)
    w[col % 5 == 0] *= np.float32(0.02)
    dst_deg = np.bincount(col, weights=w.astype(np.float64), minlength=NDST).astype(np.float32)
    src_deg = np.bincount(row, minlength=NSRC).astype(np.float32)
    src_deg[::7] = 0
    src_deg[::11] += np.float32(0.37)
    t = torch.from_numpy
    return (t(row.astype(np.int32)), t(col.astype(np.int32)), t(w), t(src_deg), t(dst_deg))


@functools.lru_cache(maxsize=4)
def tensors(dim, frame=0):
    """(hbig fp16 [NSRC, left + dim + right], obig fp32 [NDST, dim + 24]): h = columns left .. left + dim of hbig
    (normal values, a few fp16 subnormals, zeros and the largest finite value among them), the output block = columns
    8 .. 8 + dim of obig (train_refs.O_OFF), which enters holding random non-zero values"""
    left, right = H_FRAMES[frame]
    g = torch.Generator().manual_seed(104729 * frame + dim)
    hbig = torch.randn((NSRC, left + dim + right), generator=g)
    hbig[3::17] *= 1e-6          # rounds to fp16 subnormals
    hbig[5::29, ::3] = 0.0
    hbig = hbig.half()
    hbig[11, left] = 65504.0
    return hbig, torch.randn((NDST, dim + R.O_PAD), generator=g)


def h_of(hbig, dim, frame=0):
    left = H_FRAMES[frame][0]
    return hbig[:, left:left + dim]


def ex_cases():
    """(structure, dim, weighted): fgnn_block_aggregate_ex_f16 on every structure at every dim (h contiguous: the row
    stride is dim, so odd dims take the one-column path, even ones two columns per lane)"""
    return [(s, d, (i + j) % 2 == 1) for i, s in enumerate(STRUCTS) for j, d in enumerate(DIMS)]


def scaled_cases():
    """(structure, dim, frame, (src_mode, dst_mode), weighted): fgnn_block_aggregate_scaled_f16 at every dim in every
    frame (even / odd stride, even / odd base), structures and the nine mode pairs in turn, weights on two of three;
    then every mode pair on the hub block at 256 (two columns per lane) and 257 (one), with and without weights"""
    cases, i = [], 0
    for d in DIMS:
        for f in range(len(H_FRAMES)):
            cases.append((STRUCTS[i % len(STRUCTS)], d, f, MODE_PAIRS[i % 9], i % 3 != 0))
            i += 1
    for d, f in ((256, 0), (257, 1)):
        cases += [("hub_unsorted", d, f, m, j % 2 == 0) for j, m in enumerate(MODE_PAIRS)]
    return cases


def case_id(case):
    return "-".join("%d%d" % c if isinstance(c, tuple) else ("w" if c is True else "1" if c is False else str(c))
                    for c in case)
