"""The shared-key sampler (csrc/sample_khop_shared.hip) inside the batch driver, on what it takes from the single-pass
machinery: the generation wrap of the descriptor sets it stamps, the helper of its cross-workgroup prefix, one-pass
launches with 256-seed tiles, batches in flight that each list hubs in a workspace of their own.  Every batch is held to
tests/khop_shared_refs.py:reference_batch array for array, and every test shows inside its own run that its path was
taken.  The hooks and the driving loop are those of tests/test_scan_wrap_gpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import khop_shared_refs as refs
from test_coresidency_gpu import _digest
from test_hip_parity import SEED, _seeds, dev, host_u32
from test_scan_wrap_gpu import NUM_SLOTS, _assert_wrapped, _check_batch, _drive_across_generation_wrap, _forced_help

pytestmark = pytest.mark.gpu

NUM_NODE, NUM_ISOLATED = 20000, 600
SINGLE_PASS_MAX_TILES = 1536  # fgnn_device.h kSinglePassMaxTiles: above it a launch is count -> scan -> emit


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _graph(wave_row, block_row):
    """(indptr, indices, row lengths) of the module's graph"""
    rng = np.random.default_rng(41)
    live = NUM_NODE - NUM_ISOLATED
    rows = [rng.integers(0, live, int(n)) for n in rng.integers(0, 41, live)]
    special = {10: wave_row + 1, 11: wave_row + 1, 12: wave_row + 1, 13: block_row + 1, 14: block_row + 1,
               15: block_row + 1, 3: 2 * block_row + 77, 700: 4 * block_row + 1}
    for node, n in special.items():
        rows[node] = rng.integers(0, live, n)
    for i, r in enumerate(rows):
        if i in special or len(r) == 0:
            continue
        if len(r) == 1:
            r[0] = (3, 700)[i % 2]
        elif i % 7 == 0 or len(r) <= 5:
            r[:2] = 3, 700
        elif i % 11 == 0:
            r[2] = 10 + i // 11 % 6
    lens = np.zeros(NUM_NODE, dtype=np.int64)
    lens[:live] = [len(r) for r in rows]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), np.concatenate(rows).astype(np.uint32), lens


@pytest.fixture(scope="module")
def world(oracle, hip):
    """20 000 nodes.  Rows of 0 to 40 entries; the last 600 nodes have no row and are in no row (as seeds they add
    exactly themselves to a frontier).  Three rows each of wave_row + 1 and block_row + 1 entries, two hubs of 3 and 5
    pieces.  The hubs lead every seventh row and every row of at most 5 entries (rows that short are taken whole whatever
    the hubs' words are), so they are in every layer-0 frontier; the other special rows are in every eleventh row."""
    p = hip.khop_shared_params()
    indptr, indices, lens = _graph(p["wave_row"], p["block_row"])
    table = oracle.cache_table_build(np.random.default_rng(9).permutation(NUM_NODE).astype(np.uint32), NUM_NODE // 4,
                                     NUM_NODE)
    return SimpleNamespace(num_node=NUM_NODE, indptr=indptr, indices=indices, table=table, lens=lens,
                           block_row=p["block_row"])


def test_generation_wrap(hip, oracle, world):
    """eight turns of every slot: the sampler's own sets wrap between the two layers of a slot's third batch"""
    _drive_across_generation_wrap(hip, oracle, world, "khop_shared")


def test_helper_of_the_prefix(hip, oracle, world):
    """every wait that its first poll does not satisfy recomputes the missing tile's edge count (the lambda given to
    scan_prefix_help).  Layer-0 grids of about 170 to 516 tiles of 64 seeds; three turns of every slot, so the sets wrap here
    too and the helpers stamp the new cycle's generation."""
    helps0 = int(hip.load().fgnn_debug_scan_helps())
    with _forced_help(hip):
        _drive_across_generation_wrap(hip, oracle, world, "khop_shared", fanouts=[5, 10], nseed=1000, big=3000,
                                      num_batches=3 * NUM_SLOTS)
    helped = int(hip.load().fgnn_debug_scan_helps()) - helps0
    print("helped tiles:", helped)
    assert helped > 0


# ---- 256-seed tiles in one pass --------------------------------------------------------------------------------------
WIDE_FANOUTS, WIDE_MAX_BATCH = [5, 10], 9200


def _wide_cases(indptr, indices):
    """[(seeds, batch key, reference)]: layer 0's worst case n * 11 lies in (98 304, 393 216], its real frontier -- at
    most the graph's 20 000 nodes -- far below.  The second batch's frontier is a whole number of 256-seed tiles: seeds
    without a row, which no row holds, are appended until it is (and until the batch is large enough)."""
    live = NUM_NODE - NUM_ISOLATED
    out = []
    for n, num_node, key in ((9000, NUM_NODE, 61), (8700, live, 62), (8937, NUM_NODE, 63)):
        seeds = _seeds(n, num_node, seed=key)
        want = refs.reference_batch(indptr, indices, seeds, WIDE_FANOUTS, SEED, key)
        if num_node == live:
            pad = -want["graphs"][0]["num_dst"] % 256
            while n + pad < 8937:
                pad += 256
            seeds = np.concatenate([seeds, np.arange(NUM_NODE - pad, NUM_NODE, dtype=np.uint32)])
            want = refs.reference_batch(indptr, indices, seeds, WIDE_FANOUTS, SEED, key)
        out.append((seeds, key, want))
    return out


@pytest.fixture(scope="module")
def wide_cases(world):
    return _wide_cases(world.indptr, world.indices)


@pytest.mark.parametrize("forced", [False, True], ids=["plain", "helping"])
def test_one_pass_with_256_seed_tiles(hip, oracle, world, wide_cases, forced):
    """khop_shared_kernel<256> in mode 0, with most of its grid beyond the last tile (those workgroups leave without
    publishing), a frontier that ends on a tile's last seed and one that does not; plain, and with every unsatisfied
    wait helping"""
    w = world
    sampler = hip.Sampler(dev(w.indptr), dev(w.indices), WIDE_FANOUTS, WIDE_MAX_BATCH, sample_type=hip.KHOP_SHARED,
                          seed=SEED)
    bt, d_table = sampler.new_batch(), dev(w.table)
    max_tiles = hip.debug_scan_states(sampler)[0].max_tiles
    helps0 = int(hip.load().fgnn_debug_scan_helps())

    def run():
        for b, (seeds, key, want) in enumerate(wide_cases):
            assert len(seeds) <= WIDE_MAX_BATCH
            cap = len(seeds) * (1 + WIDE_FANOUTS[1])  # engine.hip: in_cap of layer 0 for this batch
            assert -(-cap // 64) > SINGLE_PASS_MAX_TILES >= -(-cap // 256) and -(-cap // 256) <= max_tiles  # S = 256, mode 0
            assert -(-len(seeds) // 64) <= SINGLE_PASS_MAX_TILES                                           # layer 1: S = 64
            frontier = want["graphs"][0]["num_dst"]
            assert frontier * 4 < cap and (frontier % 256 == 0) == (b == 1), (b, frontier)
            sampler.run_batch(b, dev(seeds), key, bt, d_table)
            _check_batch(hip, oracle, w, bt, bt.wait(), want, 2, "batch %d" % b)
    if forced:
        with _forced_help(hip):
            run()
        helped = int(hip.load().fgnn_debug_scan_helps()) - helps0
        print("helped tiles:", helped)
        assert helped > 0
    else:
        run()


# ---- batches in flight ---------------------------------------------------------------------------------------------
def test_batches_in_flight_each_list_their_own_hubs(hip, oracle, world):
    """fgnn_sampler_run_range over three streams and six buffers, every set wrapping its generation inside the first
    call while other batches are in flight.  Each slot has a hub workspace (list, pool, piece map) of its own: every
    batch's layer-0 frontier holds at least two rows beyond block_row, so overlapped batches that saw each other's lists
    or candidates would differ from the same range run one batch at a time on one stream with untouched counters
    (summaries of all batches, contents of the batches each call leaves) and from the reference (the last range)."""
    w = world
    fanouts, bs, count, chunk = [7, 5], 400, 24, 12
    limit = hip.SCAN_GEN_LIMIT
    h_train = _seeds(2400, w.num_node, seed=11)
    train, d_indptr, d_indices, d_table = dev(h_train), dev(w.indptr), dev(w.indices), dev(w.table)
    steps = len(h_train) // bs
    wants = [refs.reference_batch(w.indptr, w.indices, h_train[k * bs:(k + 1) * bs], fanouts, SEED, k) for k in range(steps)]
    for want in wants:  # hubs in every batch's layer-0 frontier
        frontier = want["input_nodes"][:want["graphs"][0]["num_dst"]]
        assert (w.lens[frontier] > w.block_row).sum() >= 2

    def run(n_streams, chunk, gens):
        sampler = hip.Sampler(d_indptr, d_indices, fanouts, bs, sample_type=hip.KHOP_SHARED, seed=SEED)
        batches = [sampler.new_batch() for _ in range(2 * n_streams)]
        streams = [torch.cuda.Stream() for _ in range(n_streams)]
        if gens:
            # per slot and turn two launches on the sampler's set and two on the table's, one per buffer: all wrap in turn two
            hip.debug_scan_set(sampler, gen=limit - 3)
            for bt in batches:
                hip.debug_scan_set(bt, gen=limit - 1)
        torch.cuda.synchronize()
        metas, digests = [], {}
        for first in range(0, count, chunk):
            ms, _, _ = sampler.run_range(first, chunk, train, bs, batches, streams, cache_table=d_table)
            assert all(m.overflow == 0 for m in ms)
            metas += [(int(m.key), int(m.num_input), int(m.num_miss), int(m.num_cache), int(m.num_edge[0]),
                       int(m.num_edge[1]), int(m.num_src[0]), int(m.num_dst[0])) for m in ms]
            for i in range(max(0, chunk - len(batches)), chunk):
                digests[first + i] = _digest(batches[(first + i) % len(batches)], ms[i], 2)
            if gens and first == 0:
                states = hip.debug_scan_states(sampler) + [s for bt in batches for s in hip.debug_scan_states(bt)]
                _assert_wrapped(states, limit - 3, "first range")
                assert all(st.gen <= 4 for st in states)
            if gens and first + chunk == count:
                for i in range(count - len(batches), count):
                    bt = batches[i % len(batches)]
                    _check_batch(hip, oracle, w, bt, bt.meta, wants[i % steps], 2, "batch %d" % i)
        torch.cuda.synchronize()
        return metas, digests

    ref_metas, ref_digests = run(1, 1, gens=False)
    metas, digests = run(3, chunk, gens=True)
    assert metas == ref_metas
    assert sorted(digests) == list(range(6, 12)) + list(range(18, 24))
    assert all(digests[i] == ref_digests[i] for i in digests), [i for i in digests if digests[i] != ref_digests[i]]
    np.testing.assert_array_equal(host_u32(d_indices), w.indices)  # the CSR is not touched
