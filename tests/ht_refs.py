"""Adversarial node-id sets, numpy mirrors of the hash functions and the plain first-occurrence reference for the two
dedup hash tables (csrc/hashtable.hip + the probes in csrc/fgnn_device.h; csrc/hashtable_partition.hip).  Plain helper
module, shared by tests/test_hashtable_adversarial_refs.py (CPU: every construction has the property it claims) and
tests/test_hashtable_adversarial_gpu.py (GPU: the kernels are held to the reference on them).  Pure numpy; nothing here
imports the kernel library or needs a GPU.

Both tables hash with (id * 0x9E3779B1) mod 2^32 and take the TOP bits: the global table's home slot is the top
log2(capacity) bits, a partitioned fill's bin the top lg bits and a key's home in its bin's LDS table the 13 bits below
those.  The multiplier is odd, hence invertible mod 2^32: any wanted hash has exactly one id (keys_for_hashes), so the
colliding sets below are constructions, not searches.  Ids of a graph (below num_node) are chosen by hashing them all.

The partition's constants come from tests/golden/partition_params.json; the GPU test checks that the library was
compiled with the same numbers (fgnn_debug_partition_params)."""
import functools
import json
import os

import numpy as np

HASH_MULT = 0x9E3779B1
HASH_INV = pow(HASH_MULT, -1, 1 << 32)
EMPTY = 0xFFFFFFFF
PARAMS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partition_params.json")))
LDS_BITS = PARAMS["lds_slots"].bit_length() - 1
NUM_NODE = 1 << 22


# ---- the hash functions -----------------------------------------------------------------------------------------------

def hash32(ids):
    return (np.asarray(ids).astype(np.uint64) * np.uint64(HASH_MULT)) & np.uint64(0xFFFFFFFF)


def keys_for_hashes(h):
    """the one 32-bit id whose hash is h, per element"""
    return ((np.asarray(h).astype(np.uint64) * np.uint64(HASH_INV)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def table_capacity(max_items):
    """fgnn_hashtable_create: the power of two >= max(1024, 2 * max_items)"""
    cap = 1024
    while cap < 2 * max_items:
        cap <<= 1
    return cap


def global_slot(ids, capacity):
    """hash_slot (fgnn_device.h)"""
    lg = capacity.bit_length() - 1
    assert capacity == 1 << lg
    return ((hash32(ids) >> np.uint64(32 - lg)) & np.uint64(capacity - 1)).astype(np.int64)


def part_log2(total, max_log2=None):
    """part_log2 (hashtable_partition.hip): log2 of the bin count of a fill of `total` = known nodes + items"""
    max_log2 = PARAMS["max_log2"] if max_log2 is None else max_log2
    want = (total + PARAMS["per_bin"] - 1) // PARAMS["per_bin"]
    lg = 0 if want <= 1 else (want - 1).bit_length()
    return min(max(lg, PARAMS["min_log2"]), max_log2)


def part_bin(ids, lg):
    """part_hist_kernel's bin: the top lg bits of the hash"""
    return (hash32(ids) >> np.uint64(32 - lg)).astype(np.int64)


def part_slot(ids, lg):
    """part_slot: the 13 hash bits below the bin's"""
    return (((hash32(ids) << np.uint64(lg)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - LDS_BITS)).astype(np.int64)


# ---- the reference -------------------------------------------------------------------------------------------------------

def first_occurrence_dedup(known, items):
    """known: the distinct ids that already have local ids 0 .. len(known) - 1; items: any ids.  New ids get local ids
    len(known) + rank in order of first occurrence.  Returns (unique_list incl. known, local id of every item)."""
    known = np.asarray(known).astype(np.int64)
    items = np.asarray(items).astype(np.int64)
    allv = np.concatenate([known, items])
    uniq, first, inv = np.unique(allv, return_index=True, return_inverse=True)
    assert len(uniq) >= len(known) and (np.sort(first)[:len(known)] == np.arange(len(known))).all(), "known not distinct"
    order = np.argsort(first, kind="stable")  # unique values by first occurrence: the known ones come first
    local_of_uniq = np.empty(len(uniq), dtype=np.int64)
    local_of_uniq[order] = np.arange(len(uniq))
    mapped = local_of_uniq[inv.reshape(-1)[len(known):]]
    return uniq[order].astype(np.uint32), mapped.astype(np.uint32)


# ---- linear probing, as far as it does not depend on the insertion order -------------------------------------------------

def probe_slots(homes, size):
    """slots that `len(homes)` distinct keys with these home slots end up occupying in a linear-probing table of `size`
    slots (the SET of slots does not depend on the insertion order).  Sorted by home; len(homes) < size."""
    h = np.sort(np.asarray(homes, dtype=np.int64))
    n = len(h)
    assert n < size
    h2 = np.concatenate([h, h + size])  # two laps: what spills over the end of the first lands at the start of the second
    i = np.arange(2 * n)
    pos = i + np.maximum.accumulate(h2 - i)
    return pos[n:] - size  # may exceed size - 1: such a key sits at slot pos - size (its chain crossed the end)


def longest_cluster(homes, size):
    """(length of the longest run of occupied slots, does a key sit below its home i.e. did a chain cross the end).  A
    probe for a key of that run walks up to `length` buckets."""
    pos = probe_slots(homes, size)
    h = np.sort(np.asarray(homes, dtype=np.int64))
    wraps = bool((pos >= size).any())
    occ = np.zeros(size, dtype=bool)
    occ[pos % size] = True
    if occ.all():
        return size, wraps
    start = int(np.flatnonzero(~occ)[0])
    r = np.roll(occ, -start)  # starts at an empty slot: no run crosses the array's end
    edges = np.diff(np.concatenate([[0], r.astype(np.int8), [0]]))
    runs = np.flatnonzero(edges == -1) - np.flatnonzero(edges == 1)
    assert (pos - h >= 0).all()
    return (int(runs.max()) if len(runs) else 0), wraps


# ---- key sets for the stand-alone table (any 32-bit id but the empty key) ---------------------------------------------------

def keys_with_homes(homes, capacity, rng):
    """distinct keys, key i with global home slot homes[i]; the low hash bits are random"""
    homes = np.asarray(homes, dtype=np.uint64)
    shift = 32 - (capacity.bit_length() - 1)
    low = rng.choice(1 << min(shift, 20), size=len(homes), replace=False).astype(np.uint64)  # distinct -> distinct keys
    keys = keys_for_hashes((homes << np.uint64(shift)) | low)
    assert (keys != EMPTY).all()
    return keys


def draw_with_repeats(rng, pool, n):
    """n items from pool, every pool element at least once, in random order"""
    assert n >= len(pool)
    items = np.concatenate([pool, rng.choice(pool, size=n - len(pool))])
    return rng.permutation(items).astype(np.uint32)


def grouped(rng, items):
    """the same multiset with the occurrences of every key next to each other (keys in random order): the items of one
    wave then race for the same few buckets, so the CAS that claims a key's bucket is often NOT its first occurrence's
    and the smaller index has to take the key over (the atomicMin / take-over note paths)"""
    items = np.asarray(items)
    uniq, inv = np.unique(items, return_inverse=True)
    return np.ascontiguousarray(items[np.argsort(rng.permutation(len(uniq))[inv.reshape(-1)], kind="stable")])


def standalone_cases():
    """{name: dict(max_items, steps=[("unique" | "dup", uint32 ids), ...], meta)}: section A of the adversarial tests.
    Built from fixed seeds: the same arrays in the CPU and the GPU test."""
    cases = {}

    def chain_case(name, seed, max_items, homes_fn):
        rng = np.random.default_rng(seed)
        cap = table_capacity(max_items)
        keys = keys_with_homes(homes_fn(rng, cap, 600), cap, rng)
        first, second, third = keys[:200], keys[200:400], keys[400:]
        f1 = draw_with_repeats(rng, np.concatenate([second, first[:100]]), 3000)
        f2 = draw_with_repeats(rng, np.concatenate([third, second[:100], first[100:]]), 3100)
        cases[name] = dict(max_items=max_items, capacity=cap, keys=keys,
                           steps=[("unique", first), ("dup", f1), ("dup", grouped(rng, f2))])

    chain_case("one_home_slot", 101, 1000, lambda rng, cap, n: np.full(n, 1023))
    chain_case("wrap_around", 102, 1000, lambda rng, cap, n: rng.integers(cap - 8, cap, size=n))

    def load_case(name, seed, max_items, n_keys, crowded):
        rng = np.random.default_rng(seed)
        cap = table_capacity(max_items)
        if crowded:
            keys = keys_with_homes(rng.integers(cap - 10, cap + 6, size=n_keys) % cap, cap, rng)  # 16 neighbouring slots
        else:
            keys = rng.choice(np.arange(1, 1 << 32, 8388593 // n_keys, dtype=np.uint64), size=n_keys,
                              replace=False).astype(np.uint32)
        items = draw_with_repeats(rng, keys[100:], 3 * n_keys)
        cases[name] = dict(max_items=max_items, capacity=cap, keys=keys,
                           steps=[("unique", keys[:100]), ("dup", items[:n_keys]), ("dup", items)])

    load_case("load_half_random", 103, 512, 512, False)
    load_case("load_half_crowded", 104, 512, 512, True)
    load_case("load_just_over_random", 105, 513, 513, False)
    load_case("load_just_over_crowded", 106, 513, 513, True)

    rng = np.random.default_rng(107)
    edge = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], dtype=np.uint32)
    high = rng.choice(np.arange(1 << 31, (1 << 32) - 2, 2003, dtype=np.uint64), size=1000, replace=False).astype(np.uint32)
    small = np.arange(2, 302, dtype=np.uint32)
    allk = np.concatenate([edge, high, small])
    cases["id_range"] = dict(max_items=2000, capacity=table_capacity(2000), keys=allk,
                             steps=[("unique", np.concatenate([edge[[3, 0]], high[:50], small[:20]])),
                                    ("dup", draw_with_repeats(rng, np.concatenate([edge, high[:600], small[:150]]), 3500)),
                                    ("dup", draw_with_repeats(rng, allk, 3900))])

    rng = np.random.default_rng(108)
    cap = table_capacity(1000)
    s = 777
    a = keys_with_homes(np.full(250, s), cap, rng)
    b = keys_with_homes(np.full(250, s + 1), cap, rng)
    inter = np.empty(500, dtype=np.uint32)
    inter[0::2], inter[1::2] = a, b
    cases["interleaved_clusters"] = dict(max_items=1000, capacity=cap, keys=inter,
                                         steps=[("dup", np.concatenate([inter, inter[::-1], inter])),
                                                ("dup", draw_with_repeats(rng, inter, 3000))])
    return cases


def generation_case():
    """section A case 5: (max_items, the 400-key single-home-slot set, per generation (unique ids, dup items))"""
    rng = np.random.default_rng(109)
    max_items = 1000
    cap = table_capacity(max_items)
    keys = keys_with_homes(np.full(400, cap - 3), cap, rng)  # the chain also crosses the table's end
    gens = []
    for g in range(21):
        sub = rng.permutation(keys)[:120 + 13 * g]  # a different subset in a different order
        gens.append((sub[:40], draw_with_repeats(rng, sub, 900 + 50 * g)))
    return dict(max_items=max_items, capacity=cap, keys=keys, gens=gens)


# ---- node ids of a graph (below NUM_NODE) by hash ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _node_hashes():
    return hash32(np.arange(NUM_NODE, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def ids_in_bin(b, lg=PARAMS["min_log2"]):
    """all node ids whose partition bin is b"""
    return np.flatnonzero((_node_hashes() >> np.uint64(32 - lg)) == b).astype(np.uint32)


def ids_in_bin_with_lds_homes(b, slots, lg=PARAMS["min_log2"]):
    ids = ids_in_bin(b, lg)
    return ids[np.isin(part_slot(ids, lg), slots)]


def ids_with_global_homes(slots, capacity):
    return np.flatnonzero(np.isin(global_slot(np.arange(NUM_NODE, dtype=np.uint64), capacity), slots)).astype(np.uint32)


def build_csr(rows):
    """{node: neighbour ids} -> (indptr, indices) uint32 over NUM_NODE nodes; all other rows are empty"""
    deg = np.zeros(NUM_NODE, dtype=np.int64)
    nodes = np.fromiter(rows.keys(), dtype=np.int64, count=len(rows))
    nodes.sort()
    deg[nodes] = [len(rows[int(n)]) for n in nodes]
    indptr = np.zeros(NUM_NODE + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.concatenate([np.asarray(rows[int(n)], dtype=np.uint32) for n in nodes] + [np.zeros(1, np.uint32)])
    return indptr.astype(np.uint32), indices


# ---- regimes of a partitioned fill ----------------------------------------------------------------------------------------------

def classify_bin(n_items, n_distinct):
    """what part_dedup_kernel does with a bin of n_items pairs (known nodes + items) holding n_distinct keys"""
    if n_items > PARAMS["hopeless_items"]:
        return "hopeless"
    if n_distinct > PARAMS["lds_slots"]:
        return "overflow"
    if n_distinct > PARAMS["lds_limit"]:
        return "limit"
    return "lds_stream" if n_items > PARAMS["reg_items"] else "lds_regs"


def fill_bins(known, items, max_log2=None):
    """per bin of the fill (known nodes + items, as part_item lays them out): dict(lg, items[B], distinct[B], regime[B],
    single_bin_tiles = histogram / scatter tiles whose items all land in one bin)"""
    flat = np.concatenate([np.asarray(known, dtype=np.uint32), np.asarray(items, dtype=np.uint32)])
    lg = part_log2(len(flat), max_log2)
    B = 1 << lg
    bins = part_bin(flat, lg)
    n_items = np.bincount(bins, minlength=B)
    ub = part_bin(np.unique(flat), lg)
    n_distinct = np.bincount(ub, minlength=B)
    tile = PARAMS["tile"]
    full = len(flat) // tile
    tb = bins[:full * tile].reshape(full, tile)
    single = int((tb == tb[:, :1]).all(axis=1).sum()) if full else 0
    return dict(lg=lg, items=n_items, distinct=n_distinct,
                regime=[classify_bin(int(i), int(d)) for i, d in zip(n_items, n_distinct)], single_bin_tiles=single)


def lds_cluster(keys, lg):
    """(longest run of occupied LDS slots, a chain crossed slot 8191 -> 0) for the distinct keys of one bin"""
    keys = np.unique(np.asarray(keys, dtype=np.uint32))
    if len(keys) >= PARAMS["lds_slots"]:
        return PARAMS["lds_slots"], True
    return longest_cluster(part_slot(keys, lg), PARAMS["lds_slots"])


def fills_of(want):
    """the fills of one oracle.do_sample result in the order the batch driver runs them (last layer first):
    [(layer, known nodes, items)] -- items are the ids the layer's sampler emitted (row is their remap)"""
    nodes = want["input_nodes"]
    out = []
    for li in range(len(want["graphs"]) - 1, -1, -1):
        g = want["graphs"][li]
        out.append((li, nodes[:g["num_dst"]], nodes[g["row"]]))
    return out


# ---- sampler cases (section B) -----------------------------------------------------------------------------------------------------

BIN_A, BIN_B, BIN_C = 7, 19, 28  # any three of the 32 bins of a fill below 65536 items
FANOUT = 160                     # rows are at most this long: khop0 / khop2 copy them whole, in CSR order


def _sub(b, lg):
    """the first of the bins that bin b of a 32-bin fill splits into when the fill has 2^lg bins"""
    return b << (lg - PARAMS["min_log2"])


def _flat_lds_chains(rng, lg, b=BIN_A):
    last = ids_in_bin_with_lds_homes(_sub(b, lg), np.arange(PARAMS["lds_slots"] - 8, PARAMS["lds_slots"]), lg)
    other = ids_in_bin_with_lds_homes(_sub(b, lg), [100, 101, 4000], lg)
    return draw_with_repeats(rng, np.concatenate([last, other]), 2400)


def _flat_hubs(rng, lg, b=BIN_A):
    return draw_with_repeats(rng, rng.choice(ids_in_bin(_sub(b, lg), lg), size=3000, replace=False), 12000)


def _flat_limit(rng, lg, b=BIN_B):
    return draw_with_repeats(rng, rng.choice(ids_in_bin(_sub(b, lg), lg), size=6600, replace=False), 6600)


def _flat_overflow(rng, lg, b=BIN_A):
    return draw_with_repeats(rng, rng.choice(ids_in_bin(_sub(b, lg), lg), size=9000, replace=False), 9000)


def _flat_hopeless(rng, lg, b=BIN_C):
    return draw_with_repeats(rng, rng.choice(ids_in_bin(_sub(b, lg), lg), size=2000, replace=False), 33600)


def _flat_mixed(rng, lg):
    # regime by regime, NOT shuffled together: whole tiles of the scatter pass then hold one bin only
    ordinary = rng.choice(NUM_NODE, size=4000).astype(np.uint32)
    return np.concatenate([_flat_lds_chains(rng, lg, BIN_A), ordinary[:2000], _flat_limit(rng, lg, BIN_B), ordinary[2000:],
                           _flat_hopeless(rng, lg, BIN_C)])


# name -> (builder of the flat item list, its length, {bin of a 32-bin fill: regime its (first sub-)bin must be in})
FLAT_CASES = {
    "lds_chains_and_wrap": (_flat_lds_chains, 2400, {BIN_A: "lds_regs"}),
    "whole_tiles_in_one_bin": (_flat_hubs, 12000, {BIN_A: "lds_stream"}),
    "limit_fall_back": (_flat_limit, 6600, {BIN_B: "limit"}),
    "real_overflow": (_flat_overflow, 9000, {BIN_A: "overflow"}),
    "hopeless": (_flat_hopeless, 33600, {BIN_C: "hopeless"}),
    "mixed": (_flat_mixed, 46600, {BIN_A: "lds_regs", BIN_B: "limit", BIN_C: "hopeless"}),
}
SHAPES = ("one_layer", "two_layers", "unit_rows")


def _chunks(flat, n):
    return [flat[i:i + n] for i in range(0, len(flat), n)]


@functools.lru_cache(maxsize=None)
def sampler_case(name, shape):
    """Two batches (own seeds, mids and item lists) on one graph of NUM_NODE nodes; the adversarial ids are the `flat`
    list of the case.
      one_layer   fanouts [FANOUT]: the seeds' rows are the flat list cut into rows (khop0 / khop2 copy rows of at most
                  `fanout` entries whole, in CSR order: the fill's items are exactly the flat list)
      two_layers  fanouts [FANOUT, 24]: each seed's row is 24 `mid` nodes, the mids' rows are the flat list -- it arrives in
                  the LAST fill (layer 0), behind the re-emitted mids
      unit_rows   fanouts [2, 2], for the with-replacement samplers: seed i's row is [mid i], mid i's row is [flat[i]];
                  every draw of a row of one entry picks it and the sampler drops the repeats, so the last fill's items
                  are the mids (all known by then) followed by the flat list, item for item
    Returns dict(indptr, indices, fanouts, batches=[seeds, seeds], max_batch, lg = log2 bins of the adversarial fill,
    expect = {bin: regime})."""
    build, n_flat, expect = FLAT_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 8 + SHAPES.index(shape))
    lg = part_log2(4 * n_flat) if shape == "unit_rows" else PARAMS["min_log2"]
    rows, batches = {}, []
    free = rng.permutation(NUM_NODE)[:200000].astype(np.uint32)  # ordinary ids for the nodes that have rows
    used = 0
    for b in range(2):
        flat = build(rng, lg)
        assert len(flat) == n_flat
        flat_rows = _chunks(flat, 1 if shape == "unit_rows" else FANOUT)
        n_seed = {"one_layer": 0, "two_layers": -(-len(flat_rows) // 24), "unit_rows": len(flat_rows)}[shape]
        ids = free[used:used + len(flat_rows) + n_seed]
        used += len(ids)
        if shape == "unit_rows":
            # the with-replacement samplers emit their edges ordered by source id: seeds below mids, mids ascending, so
            # that the last fill's items are the re-emitted mids and then the flat list in ITS order
            ids = np.sort(ids)
        seeds, front = ids[:n_seed], ids[n_seed:]
        for n, r in zip(front, flat_rows):
            rows[int(n)] = r
        for n, r in zip(seeds, _chunks(front, 1 if shape == "unit_rows" else 24)):
            rows[int(n)] = r
        batches.append(seeds if n_seed else front)
    indptr, indices = build_csr(rows)
    fanouts = {"one_layer": [FANOUT], "two_layers": [FANOUT, 24], "unit_rows": [2, 2]}[shape]
    return dict(indptr=indptr, indices=indices, fanouts=fanouts, batches=batches, max_batch=max(len(s) for s in batches),
                lg=lg, expect={_sub(b, lg): r for b, r in expect.items()})


CROSS_CASES = ("falls_back_twice", "falls_back_then_lds")


@functools.lru_cache(maxsize=None)
def cross_fill_case(name):
    """khop1 (`table_free`: every fill partitioned, the global table only written by fall-backs), 6600 seeds, seed i's row
    is [mid i], the 6600 distinct mids all sit in bin BIN_A of a 32-bin fill: the FIRST fill's bin BIN_A holds more than
    lds_limit distinct keys and falls back, leaving its new keys pending in the global table.  The last fill re-emits
    the mids, now known nodes, as its first 6600 items.
      falls_back_twice     fanouts [2, 2], a mid's row is one ordinary id: the last fill has 32 bins again, BIN_A holds
                           the 6600 known mids and falls back again -- the pending values of the first fill meet the
                           local ids in the global table
      falls_back_then_lds  fanouts [10, 2], a mid's row is 10 ordinary ids: the last fill is large enough for 64 bins, the
                           mids split evenly over the two halves of BIN_A and both stay LDS-resident -- what the first
                           fill left in the global table must not matter
    The reverse order (LDS-resident in the first fill, fall-back in the last) is every fall-back case of
    sampler_case(..., "unit_rows")."""
    rng = np.random.default_rng(900 + CROSS_CASES.index(name))
    f0 = 2 if name == "falls_back_twice" else 10
    row_len = 1 if name == "falls_back_twice" else 10
    lg_last = PARAMS["min_log2"] + (name == "falls_back_then_lds")
    free = rng.permutation(NUM_NODE).astype(np.uint32)
    halves = [ids_in_bin(_sub(BIN_A, 6) + h, 6) for h in (0, 1)]
    free = free[~np.isin(free, np.concatenate(halves))][:2 * (6600 + 6600 * row_len)]
    rows, batches, used = {}, [], 0
    for b in range(2):
        mids = rng.permutation(np.concatenate([rng.choice(h, size=3300, replace=False) for h in halves]))
        seeds = free[used:used + 6600]
        used += 6600
        for s, m in zip(seeds, mids):
            rows[int(s)] = [m]
        for m in mids:
            rows[int(m)] = free[used:used + row_len]  # (a mid of both batches keeps the second batch's row)
            used += row_len
        batches.append(seeds)
    indptr, indices = build_csr(rows)
    last = ({BIN_A: "limit"} if name == "falls_back_twice" else
            {_sub(BIN_A, 6): "lds_stream", _sub(BIN_A, 6) + 1: "lds_stream"})
    return dict(indptr=indptr, indices=indices, fanouts=[f0, 2], batches=batches, max_batch=6600, lg=lg_last, expect=last,
                expect_first=(PARAMS["min_log2"], {BIN_A: "limit"}))


def predict_num_nodes(batch, fanouts):
    n = batch
    for f in reversed(fanouts):
        n += n * f
    return n


@functools.lru_cache(maxsize=None)
def global_collision_case():
    """section B case 7, fanouts [FANOUT, 24]: the mids (first-sampled layer) and the ids of their rows (last layer) all
    have their home in 12 slots of the sampler's global table, 6 either side of its end.  Those slots share the hash's
    top bits, so the last layer's ids also sit in one or two partition bins."""
    rng = np.random.default_rng(77)
    fanouts, n_seed = [FANOUT, 24], 2
    max_nodes = predict_num_nodes(n_seed, fanouts)
    cap = table_capacity(max_nodes)
    pool = rng.permutation(ids_with_global_homes((np.arange(cap - 6, cap + 6) % cap), cap))
    rows, batches, used = {}, [], 0
    seeds_all = rng.permutation(NUM_NODE)[:2 * n_seed].astype(np.uint32)
    assert not np.isin(seeds_all, pool).any()
    for b in range(2):
        mids = pool[used:used + 24 * n_seed]
        used += len(mids)
        rest = pool[used:]  # never a mid of this batch; mids of the other batch may be among them (then known or not)
        for m in mids:
            rows[int(m)] = rng.choice(rest[:500], size=FANOUT).astype(np.uint32)
        seeds = seeds_all[b * n_seed:(b + 1) * n_seed]
        for s, g in zip(seeds, _chunks(mids, 24)):
            rows[int(s)] = g
        batches.append(seeds)
    indptr, indices = build_csr(rows)
    return dict(indptr=indptr, indices=indices, fanouts=fanouts, batches=batches, max_batch=n_seed, capacity=cap,
                max_nodes=max_nodes, pool=pool)


# ---- the oracle over a sampler case, and what its output must show (shared by the CPU and the GPU test) ---------------------

SAMPLER_KINDS = {"one_layer": "KHOP0", "two_layers": "KHOP2", "unit_rows": "KHOP1"}
LDS_REGIMES = ("lds_regs", "lds_stream")


def sampler_regimes(oracle, case, kind, seed=0x5A4D47, want_out=None):
    """runs the oracle over the case's two batches; per batch the fill_bins of the last fill (layer 0) with, for every
    expected bin, its LDS cluster and how many of its items repeat a known node; under "first" the fill_bins of the
    first fill of a two-layer batch.  Shared with the GPU test (which passes want_out to keep the oracle's results).
    The bin count is not clamped below the library's largest: a table's own largest (partition_create) is the first
    power of two with per_bin * bins >= max_items + max_fill_items, and a fill the partition accepts (partition_fits)
    has no more than that many known nodes + items, so part_log2 never asks for more bins than the table has."""
    max_nodes = predict_num_nodes(case["max_batch"], case["fanouts"])
    oht = oracle.HashTable(NUM_NODE, max_nodes)
    rng = oracle.make_rng(oracle.RNG_PHILOX, seed)
    indices = case["indices"].copy()
    out = []
    for b, seeds in enumerate(case["batches"]):
        want = oracle.do_sample(case["indptr"], indices, seeds, case["fanouts"], getattr(oracle, kind), rng, 40 + b, oht)
        if want_out is not None:
            want_out.append(want)
        fills = fills_of(want)
        li, known, items = fills[-1]
        assert li == 0
        fb = fill_bins(known, items)
        flat = np.concatenate([known, items])
        bins_flat, bins_items = part_bin(flat, fb["lg"]), part_bin(items, fb["lg"])
        fb["clusters"] = {bn: lds_cluster(flat[bins_flat == bn], fb["lg"]) for bn in case["expect"]}
        fb["known_again"] = {bn: int(np.isin(items[bins_items == bn], known).sum()) for bn in case["expect"]}
        fb["total"] = len(flat)
        fb["first"] = None
        if len(fills) == 2:
            _, known1, items1 = fills[0]
            first = fb["first"] = fill_bins(known1, items1)
            first["total"] = len(known1) + len(items1)
            # nodes that were NEW in the first fill and sat in a bin of it that fell back: the global table holds them
            # with the pending value of that fill.  How many items of the last fill name one of them, per expected bin
            new1 = known[len(known1):]
            fell = new1[~np.isin(np.asarray(first["regime"])[part_bin(new1, first["lg"])], LDS_REGIMES)]
            fb["left_pending_again"] = {bn: int(np.isin(items[bins_items == bn], fell).sum()) for bn in case["expect"]}
        out.append(fb)
    assert (indices == case["indices"]).all()  # no row is longer than its fanout: khop2 rewrites nothing
    return out


def check_regimes(name, case, fills):
    lg_first, expect_first = case.get("expect_first", (None, {}))
    for fb in fills:
        assert fb["lg"] == case["lg"], (name, fb["lg"])
        for bn, regime in case["expect"].items():
            assert fb["regime"][bn] == regime, (name, bn, fb["regime"][bn], int(fb["items"][bn]), int(fb["distinct"][bn]))
        others = [r for bn, r in enumerate(fb["regime"]) if bn not in case["expect"]]
        assert set(others) <= {"lds_regs"}, name  # the ordinary bins
        first = fb["first"]
        assert (first is not None) == (len(case["fanouts"]) == 2)
        if first is not None:  # the first fill: its expected bins in their regime, every other bin LDS-resident
            assert lg_first is None or first["lg"] == lg_first, (name, first["lg"])
            for bn, regime in expect_first.items():
                assert first["regime"][bn] == regime, (name, "first fill", bn, first["regime"][bn])
            assert {r for bn, r in enumerate(first["regime"]) if bn not in expect_first} <= {"lds_regs"}, name
        if name in CROSS_CASES:
            # the first fill's fall-back left the mids pending in the global table; the last fill names each of them again
            assert sum(fb["left_pending_again"].values()) == 6600, (name, fb["left_pending_again"])
            assert min(fb["left_pending_again"].values()) >= 3000 or len(case["expect"]) == 1
        elif case["fanouts"] == [2, 2]:
            # a bin that falls back in the last fill was LDS-resident in the first: its known nodes never reached the global
            # table, and some of the bin's items name them
            for bn, regime in case["expect"].items():
                if regime not in LDS_REGIMES:
                    assert fb["known_again"][bn] >= 100 and fb["left_pending_again"][bn] == 0, (name, bn)
        if name in ("lds_chains_and_wrap", "mixed"):
            bn = next(iter(case["expect"]))
            length, wraps = fb["clusters"][bn]
            # one run of occupied slots across slot 8191 -> 0: the last 8 slots are the home of ~131 node ids of a bin at
            # 32 bins and of ~33 at 128
            assert wraps and length >= (100 if fb["lg"] == 5 else 30), (name, length, wraps)
            assert fb["distinct"][bn] < PARAMS["lds_limit"] // 4
        if name in ("whole_tiles_in_one_bin", "hopeless", "mixed", "real_overflow"):
            assert fb["single_bin_tiles"] >= 1, name  # a histogram / scatter tile with one bin only


def global_collision_stats(case, want):
    """(longest cluster in the sampler's global table, chain crosses its end) for the nodes of one batch"""
    nodes = want["input_nodes"]
    return longest_cluster(global_slot(nodes, case["capacity"]), case["capacity"])
