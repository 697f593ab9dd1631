"""References for the 8-bit feature store (csrc/q8_rows.h: a row of D columns is S = round_up(D, 16) + 16 bytes -- D
codes, zeros, then scale and lo as fp32 and eight zero bytes).  Plain numpy, nothing imports the kernel library: the
encode in float32 operations in the order the format fixes, the decode as the kernels document it (one float32 multiply,
one float32 add), and the float64 aggregation over the exactly decoded rows with its bound."""
import numpy as np

U23 = 2.0 ** -23


def row_bytes(dim):
    return (dim + 15) // 16 * 16 + 16


def encode(x):
    """uint8 [n, S] of float32 x [n, D], row by row"""
    x = np.asarray(x, dtype=np.float32)
    n, dim = x.shape
    S = row_bytes(dim)
    rows = np.zeros((n, S), dtype=np.uint8)
    for i in range(n):
        lo, hi = x[i].min(), x[i].max()
        scale = np.float32(0)
        if hi != lo:
            scale = np.float32(hi - lo) / np.float32(255)
            inv = np.float32(255) / np.float32(hi - lo)
            rows[i, :dim] = np.minimum(255, np.maximum(0, np.rint((x[i] - lo) * inv))).astype(np.uint8)
        rows[i, S - 16:S - 8] = np.array([scale, lo], dtype=np.float32).view(np.uint8)
    return rows


def parts(rows, dim):
    """(codes uint8 [n, D], scale float32 [n, 1], lo float32 [n, 1]) of q8 rows"""
    S = row_bytes(dim)
    hdr = np.ascontiguousarray(rows[:, S - 16:S - 8]).view(np.float32)
    return rows[:, :dim], hdr[:, :1], hdr[:, 1:2]


def decode_f32(rows, dim):
    """lo + scale * q in float32: the multiply rounded, then the add rounded -- what the kernels compute"""
    q, scale, lo = parts(rows, dim)
    prod = scale * q.astype(np.float32)
    assert prod.dtype == np.float32
    return lo + prod


def roundtrip_bound(rows, dim):
    """per element: the code's half step, plus the float32 rounding of the encode's subtract and multiply and of the
    decode"""
    _, scale, lo = parts(rows, dim)
    scale, lo = scale.astype(np.float64), lo.astype(np.float64)
    return scale / 2 + 2.0 ** -22 * (np.abs(lo) + 255 * scale)


def degree_factor(deg, mode):
    d = np.maximum(np.asarray(deg, dtype=np.float64), 1)
    return np.ones_like(d) if mode == 0 else (d ** -0.5 if mode == 1 else 1 / d)


def aggregate(src, dst, w, rows, dim, num_dst, src_deg=None, src_mode=0, dst_deg=None, dst_mode=0):
    """(ref, bound) in float64 for out[dst[e]] += f_dst w_e f_src (lo + scale q) of row src[e]: the sum over the exactly
    decoded rows, and (2 k + 8) 2^-23 times the sum of the magnitudes of its 2 k terms per column, |w f scale q| and
    |w f lo| times the destination factor, k = the destination's edge count"""
    q, scale, lo = (a.astype(np.float64) for a in parts(rows, dim))
    f = np.ones(len(src)) if w is None else np.asarray(w, dtype=np.float64)
    if src_mode:
        f = f * degree_factor(src_deg, src_mode)[src]
    f = f[:, None]
    ref, mag = np.zeros((num_dst, dim)), np.zeros((num_dst, dim))
    np.add.at(ref, dst, f * (lo[src] + scale[src] * q[src]))
    np.add.at(mag, dst, np.abs(f * scale[src] * q[src]) + np.abs(f * lo[src]))
    fd = degree_factor(dst_deg, dst_mode)[:, None] if dst_mode else 1.0
    k = np.bincount(dst, minlength=num_dst)[:, None]
    return fd * ref, (2 * k + 8) * U23 * fd * mag


def features(n, dim, seed):
    """float32 [n, D]: rows of different scales and offsets (negative, positive and mixed ranges), one constant row"""
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n, dim)) * rs.choice([1e-3, 1.0, 40.0], (n, 1)) + rs.choice([-7.0, 0.0, 3.5], (n, 1))
    x = x.astype(np.float32)
    x[n // 2] = np.float32(1.5)
    return x
