"""References for the feature-movement kernels of csrc/cache_gather.hip (fgnn_gather_rows / _masked / _shared,
fgnn_extract_fused, fgnn_get_miss_cache_index, the label tail) and for the 32-bit tile walk of its chunk kernels.

 * gather_ref: out[dst[i] or i] = src[(idx[i] or i) & mask] for i < n, on rows of bytes (numpy); split_ref: the stable
   partition of a node list by table[node] != EMPTY.  Both are what the kernels must equal byte for byte.
 * GATHER_CASES: the pairwise case table of the stand-alone gathers, shared by tests/test_gather_references.py (which
   shows that it covers every axis value and every path x count-source pair, and that no case addresses memory outside
   its buffers) and tests/test_gather_paths_gpu.py (which runs it).  build_gather_case lays a case out in memory.
 * simulate_walk: the tile walk of gather_rows16_kernel / gather_band in integers modulo 2^32, one workgroup at a time.
   A walk is wrong when a workgroup comes back to a tile it has visited (it then never ends), when a tile is visited
   twice or not at all, or when the ragged tail has no or several takers -- the verdict is the revisit itself, never a
   step count.  check_plan applies it to every launch of an fgnn_debug_gather_plan answer.
"""
import collections
import functools

import numpy as np

EMPTY = 0xFFFFFFFF
NO_MASK = 0xFFFFFFFF
SPAN = 1 << 32            # what a 32-bit cursor can tell apart
KBLOCK = 256              # threads of a workgroup (fgnn_device.h kBlock)
VEC_UNROLL = 4            # 16-byte loads per lane of the shipped chunk gather: a tile is KBLOCK * VEC_UNROLL chunks
VEC_WG_PER_CU = 4         # grid cap of fgnn_gather_rows*: persistent workgroups per CU of the chunk kernel ...
ELEM_WG_PER_CU = 16       # ... and of the element kernel (one element per thread and trip)
ITEMS_PER_THREAD = 8      # fgnn_get_miss_cache_index beyond 4 << 20 nodes (kItemsPerThread)
MAX_COPY_SEGMENTS = 32    # FGNN_MAX_COPY_SEGMENTS
POISON = 0xA5             # every output byte before a launch
GUARD_ROWS = 8            # untouched rows before and after every output

# dtype codes of fgnn_hip/lib.py (F32, F64, F16, U8, I32, I8, I64 = 0 .. 6) and their element sizes
DTYPES = {"F32": (0, 4), "F64": (1, 8), "F16": (2, 2), "U8": (3, 1), "I32": (4, 4), "I8": (5, 1), "I64": (6, 8)}


# ---- references --------------------------------------------------------------------------------------------------------------

def gather_ref(out_rows, src_rows, n, idx=None, dst=None, mask=NO_MASK):
    """out_rows[dst[i] or i] = src_rows[(idx[i] or i) & mask] for i < n, in place; rows are uint8[rows, row_bytes]"""
    assert out_rows.dtype == np.uint8 and src_rows.dtype == np.uint8 and out_rows.shape[1] == src_rows.shape[1]
    i = np.arange(n, dtype=np.int64)
    s = (idx[:n].astype(np.int64) if idx is not None else i) & mask
    d = dst[:n].astype(np.int64) if dst is not None else i
    assert len(np.unique(d)) == n, "destinations must be distinct: the result would depend on the order of the writes"
    out_rows[d] = src_rows[s]
    return out_rows


def split_ref(table, nodes):
    """(miss_src, miss_dst, cache_src, cache_dst): stable partition of nodes[] by table[node] != EMPTY -- a miss keeps
    its node id and position, a hit its cache slot and position"""
    slot = table[nodes]
    pos = np.arange(len(nodes), dtype=np.uint32)
    miss = slot == EMPTY
    return nodes[miss], pos[miss], slot[~miss], pos[~miss]


def cache_table(num_node, frac, seed):
    """(table, rank): table[rank[i]] = i for the first frac * num_node nodes of a random ranking, EMPTY elsewhere"""
    rank = np.random.default_rng(seed).permutation(num_node).astype(np.uint32)
    n_cached = int(num_node * frac)
    table = np.full(num_node, EMPTY, np.uint32)
    table[rank[:n_cached]] = np.arange(n_cached, dtype=np.uint32)
    return table, rank


# ---- the 32-bit tile walk ----------------------------------------------------------------------------------------------------

def parent_rule(total):
    """what the launchers admitted before the planner: any chunk total below 0xffffffff, whatever the grid"""
    return total < 0xFFFFFFFF


def admissible(total, grid, tile):
    """the planner's rule, restated: the last addition of any workgroup's cursor stays within 32 bits"""
    return total + grid * tile <= SPAN


_STEPS = 4096  # cursor positions computed per numpy call (a block size, not a verdict)


_KS = np.arange(_STEPS, dtype=np.int64)


def _walk_one(b, full, step, tile, owner, hits, step_of):
    """Workgroup b's walk.  owner[t]: the last workgroup that took tile t (-1: none yet), hits[t]: how often it was
    taken, step_of[t]: scratch.  Returns where the cursor ends, or ('revisit', tile) when the workgroup comes back to a
    tile it has taken itself -- from there on it repeats itself for ever."""
    pos = (b * tile) % SPAN
    while True:
        p = (pos + _KS * step) % SPAN  # (below 2^44: exact in int64)
        out = np.nonzero(p >= full)[0]
        t = (p[:out[0]] if len(out) else p) // tile
        if len(t):
            mine = owner[t] == b
            if mine.any():
                return ("revisit", int(t[np.argmax(mine)]))
            owner[t] = b
            step_of[t] = _KS[:len(t)]              # a tile taken twice within this block keeps the later step only
            twice = step_of[t] != _KS[:len(t)]
            if twice.any():
                return ("revisit", int(t[np.argmax(twice)]))
            hits[t] += 1
        if len(out):
            return int(p[out[0]])
        pos = (int(p[-1]) + step) % SPAN


@functools.lru_cache(maxsize=None)
def simulate_walk(total, grid, tile):
    """None when `grid` workgroups walking `total` chunks in tiles of `tile` as the kernels do (cursor = b * tile,
    += grid * tile while below the last whole tile's end, all modulo 2^32) visit every whole tile exactly once, all
    end, and exactly one of them takes the ragged tail (none when there is no tail); else a sentence saying what goes
    wrong"""
    if total >= SPAN:
        return "the chunk total %#x does not fit the kernel's 32-bit `total`" % total
    if grid < 1 or SPAN % tile:
        return "no grid, or a tile that does not divide 2^32"
    full = total // tile * tile
    step = (grid * tile) % SPAN
    ntiles = full // tile
    hits, owner, step_of = np.zeros(ntiles, np.uint8), np.full(ntiles, -1, np.int32), np.zeros(ntiles, np.int64)
    tails = 0
    for b in range(grid):
        end = _walk_one(b, full, step, tile, owner, hits, step_of)
        if isinstance(end, tuple):
            return "workgroup %d revisits tile %d and never ends" % (b, end[1])
        tails += end == full and full < total
    if len(hits) and (hits.min() != 1 or hits.max() != 1):
        return "tile %d is visited %d times" % (int(np.argmax(hits != 1)), int(hits[np.argmax(hits != 1)]))
    if tails != (1 if full < total else 0):
        return "%d workgroups take the ragged tail" % tails
    return None


def check_plan(plan, rows, cpr, grid_cap, tile):
    """a plan (list of (first_row, rows, grid, tile)) covers [0, rows) exactly once and in order, sizes every launch as
    the launcher does, and every launch's walk is sound"""
    at = 0
    for first, count, grid, t in plan:
        assert first == at and count > 0 and t == tile, (first, count, grid, t)
        assert grid == min(-(-count * cpr // tile), grid_cap), (count, grid)
        bad = simulate_walk(count * cpr, grid, tile)
        assert bad is None, "launch (%d rows of %d chunks, grid %d, tile %d): %s" % (count, cpr, grid, tile, bad)
        at += count
    assert at == rows, (at, rows)


# ---- the stand-alone gathers' case table -------------------------------------------------------------------------------------
# dtype; row bytes (0: one element); index form; where the count comes from (H: host n, LT: d_n < cap, Z: d_n = 0, GT:
# d_n > cap, clamped); mask (none / pow2: 2^k - 1 with ids beyond the table / noindex: a mask without a source index);
# misalignment (which base pointer, bytes off a 16-byte boundary); row count (one; tile-1 / tile / tile+1: a total of
# one tile of the path's walk, give or take one unit where the row width allows it, else the nearest row count; ktiles:
# exactly k tiles, no ragged tail; trip2: beyond twice the path's grid cap, so that the grid-stride loop goes round again)
GatherCase = collections.namedtuple("GatherCase", "dtype row_bytes form count mask align rows")
_C = GatherCase
GATHER_CASES = [
    # the compiled 25 chunks per row
    _C("F32", 400, "src", "H", "none", None, "trip2"),
    _C("F16", 400, "both", "LT", "pow2", None, "ktiles"),
    _C("F64", 400, "dst", "Z", "none", None, "tile"),
    _C("I32", 400, "neither", "GT", "noindex", None, "one"),
    # the compiled 32
    _C("I64", 512, "both", "H", "none", None, "tile"),
    _C("U8", 512, "src", "LT", "none", None, "tile+1"),
    _C("F32", 512, "neither", "Z", "none", None, "one"),
    _C("F16", 512, "dst", "GT", "noindex", None, "ktiles"),
    # the compiled 64
    _C("I8", 1024, "dst", "H", "noindex", None, "ktiles"),
    _C("F64", 1024, "both", "LT", "pow2", None, "tile-1"),
    _C("I32", 1024, "src", "Z", "pow2", None, "tile"),
    _C("F32", 1024, "neither", "GT", "none", None, "tile+1"),
    # the generic chunk kernel: 1, 3, 65 and 1025 chunks per row (the last is wider than a tile)
    _C("F32", 16, "src", "H", "none", None, "tile-1"),
    _C("F32", 16, "both", "H", "none", None, "tile"),
    _C("I32", 16, "dst", "H", "none", None, "tile+1"),
    _C("F16", 48, "neither", "LT", "none", None, "ktiles"),
    _C("I64", 1040, "src", "Z", "none", None, "one"),
    _C("F64", 16400, "both", "GT", "pow2", None, "tile+1"),
    _C("U8", 16400, "src", "H", "none", None, "one"),
    _C("I8", 16, "src", "LT", "pow2", None, "trip2"),
    # the element kernel: rows that are not whole chunks ...
    _C("U8", 0, "src", "H", "none", None, "trip2"),
    _C("I8", 12, "both", "LT", "none", None, "tile"),
    _C("F16", 0, "dst", "Z", "none", None, "tile"),
    _C("F32", 12, "neither", "GT", "noindex", None, "tile+1"),
    _C("I32", 0, "src", "GT", "pow2", None, "one"),
    _C("F64", 0, "both", "H", "pow2", None, "tile-1"),
    _C("I64", 0, "dst", "LT", "none", None, "ktiles"),
    # ... and whole-chunk rows behind a base pointer that is not 16-byte aligned
    _C("F32", 512, "src", "H", "none", ("out", 4), "ktiles"),
    _C("F16", 1024, "both", "LT", "none", ("out", 8), "tile"),
    _C("I32", 400, "dst", "H", "none", ("src", 4), "tile+1"),
    _C("F64", 16, "src", "H", "none", ("src", 8), "tile-1"),
    _C("U8", 48, "neither", "GT", "none", ("out", 4), "one"),
]

AXES = {
    "dtype": ["U8", "I8", "F16", "F32", "I32", "F64", "I64"],
    "row_bytes": [0, 12, 16, 48, 400, 512, 1024, 1040, 16400],
    "form": ["src", "dst", "both", "neither"],
    "count": ["H", "LT", "Z", "GT"],
    "mask": ["none", "pow2", "noindex"],
    "align": [None, ("out", 4), ("out", 8), ("src", 4), ("src", 8)],
    "rows": ["one", "tile-1", "tile", "tile+1", "ktiles", "trip2"],
}
PATHS = ["cpr25", "cpr32", "cpr64", "generic", "elem"]


def case_row_bytes(case):
    return case.row_bytes or DTYPES[case.dtype][1]


def case_path(case):
    """which kernel the launcher must choose: the element kernel for rows that are not whole 16-byte chunks AND for any
    base pointer off a 16-byte boundary, else the chunk kernel compiled for 25 / 32 / 64 chunks per row or the generic"""
    rb = case_row_bytes(case)
    if rb % 16 or case.align:
        return "elem"
    return {25: "cpr25", 32: "cpr32", 64: "cpr64"}.get(rb // 16, "generic")


def case_id(case):
    return "-".join([case.dtype, "%dB" % case_row_bytes(case), case.form, case.count, case.mask,
                     "%s+%d" % case.align if case.align else "aligned", case.rows, case_path(case)])


def case_rows(case, cus):
    """the row count the case's `rows` stands for on a device of `cus` compute units: the unit of the path's walk is a
    16-byte chunk and a tile of KBLOCK * VEC_UNROLL of them under a cap of VEC_WG_PER_CU * cus workgroups, or an element
    and KBLOCK of them under ELEM_WG_PER_CU * cus"""
    rb = case_row_bytes(case)
    if case_path(case) == "elem":
        per_row, tile, cap = rb // DTYPES[case.dtype][1], KBLOCK, ELEM_WG_PER_CU * cus
    else:
        per_row, tile, cap = rb // 16, KBLOCK * VEC_UNROLL, VEC_WG_PER_CU * cus
    if case.rows == "one":
        return 1
    if case.rows == "ktiles":  # the smallest k > 1 tiles that are whole rows
        k = 2
        while k * tile % per_row:
            k += 1
        return k * tile // per_row
    if case.rows == "trip2":
        return (2 * cap * tile + 3 * tile + tile // 2) // per_row + 1
    units = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[case.rows]
    return max(1, -(-units // per_row) if case.rows == "tile+1" else units // per_row)


GatherLayout = collections.namedtuple(
    "GatherLayout", "row_bytes dim n n_host d_n cap src idx dst mask out_rows body want src_off out_off")


def build_gather_case(case, cus, seed=0):
    """Lays a case out.  src: uint8[src rows, row_bytes] of random bytes; idx / dst: uint32[cap] or None; out_rows: rows
    of the output buffer including GUARD_ROWS before and after its body, every byte POISON; body: first row of the
    body; want: the output buffer after the launch.  Entries of idx / dst beyond a device-side count are VALID row
    numbers whose destination is a guard row after the body, so a kernel that reads past its count changes a guard
    row -- nothing addresses memory outside src and the output buffer."""
    rs = np.random.default_rng(1000 + seed)
    rb = case_row_bytes(case)
    rows = case_rows(case, cus)
    # the count the launch must honour, the capacity it is sized for and what the host and the device say
    if case.count == "H":
        n, cap, n_host, d_n = rows, rows, rows, None
    elif case.count == "LT":
        n, cap, n_host, d_n = rows, rows + 37, 0, rows
    elif case.count == "Z":
        n, cap, n_host, d_n = 0, rows, 0, 0
    else:
        n, cap, n_host, d_n = rows, rows, 0, rows + 1000
    has_src, has_dst = case.form in ("src", "both"), case.form in ("dst", "both")
    mask = NO_MASK if case.mask == "none" else 63
    if case.mask != "none":
        n_src = 64                                    # a 2^k-row table (the reference's SAMGRAPH_EMPTY_FEAT mock)
    else:
        n_src = 257 if has_src else cap
    src = rs.integers(0, 256, size=(n_src, rb), dtype=np.uint8)
    idx = None
    if has_src:
        idx = rs.integers(0, 1 << 20 if case.mask == "pow2" else n_src, size=cap).astype(np.uint32)
        idx[n:] = 0 if case.mask != "pow2" else 64 * 5 + 1  # beyond the count: valid (masked) row numbers
    body_rows = cap + 13 if has_dst else cap
    dst = None
    if has_dst:
        dst = np.empty(cap, np.uint32)
        dst[:n] = rs.permutation(body_rows)[:n]
        dst[n:] = body_rows + np.arange(cap - n) % GUARD_ROWS  # beyond the count: a guard row after the body
    out_rows = GUARD_ROWS + body_rows + GUARD_ROWS
    want = np.full((out_rows, rb), POISON, np.uint8)
    gather_ref(want[GUARD_ROWS:GUARD_ROWS + body_rows], src, n, idx, dst, mask)
    src_off = case.align[1] if case.align and case.align[0] == "src" else 0
    out_off = case.align[1] if case.align and case.align[0] == "out" else 0
    return GatherLayout(rb, rb // DTYPES[case.dtype][1], n, n_host, d_n, cap, src, idx, dst, mask, out_rows,
                        GUARD_ROWS, want, src_off, out_off)


def layout_stays_inside(lay):
    """every row a launch of this layout may read or write -- for ANY count up to the capacity -- lies in its buffers"""
    i = np.arange(lay.cap, dtype=np.int64)
    s = (lay.idx.astype(np.int64) if lay.idx is not None else i) & lay.mask
    d = lay.dst.astype(np.int64) if lay.dst is not None else i
    return bool((s < len(lay.src)).all() and (lay.body + d < lay.out_rows).all())
