"""The shared-key sampler (csrc/sample_khop_shared.hip, sample type 8) against tests/khop_shared_refs.py, for equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import khop_shared_refs as refs
from fgnn_hip import lib as hip

pytestmark = pytest.mark.gpu
SEED, NUM_NODE = 0x5A4D47, 40000


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def u32(t, n=None):
    return t.cpu().numpy().view(np.uint32)[:n]


def _graph(rows, num_node):
    lens = np.zeros(num_node, dtype=np.int64)
    lens[:len(rows)] = [len(r) for r in rows]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    return indptr, np.concatenate(rows).astype(np.uint32)


def _edge_case_graph(k, p):
    """one row per length at which a path can go wrong for fanout k, then the rows with special contents"""
    rng = np.random.default_rng(k)
    wave, block = p["wave_row"], p["block_row"]
    lens = [0, 1, max(k - 1, 0), k, k + 1, 63, 64, 65, wave - 1, wave, wave + 1, block - 1, block, block + 1,
            3 * block + 17]
    rows = [rng.integers(0, NUM_NODE, n) for n in lens]
    rows += [np.full(2 * k + 2, 777),                          # one neighbour id more than k times: ties by position
             rng.choice([5, 6], 3 * 64 + 9),                   # ties across a wave's trips
             rng.choice([5, 6, 7], wave + 900),                # ... in the workgroup's path
             rng.choice([5, 6, 7, 8, 9], 2 * block + 100),     # ... across a hub's pieces
             rng.integers(0, NUM_NODE // 4, 200) * 4,          # ids all 0 mod 4: word 0 of distinct blocks
             np.tile(np.arange(4000, 4004), 30)]               # four consecutive ids: the four words of one block
    seeds = np.concatenate([np.arange(len(rows)), [4, 14, 14]]).astype(np.uint32)  # nodes twice, a hub among them
    return _graph(rows, NUM_NODE) + (seeds,)


@pytest.mark.parametrize("fanout", [1, 5, 25, "limit"])
def test_stateless_entry_point_equals_the_reference(fanout):
    p = hip.khop_shared_params()
    k = p["max_fanout"] if fanout == "limit" else fanout
    indptr, indices, seeds = _edge_case_graph(k, p)
    d_indptr, d_indices, d_seeds = dev(indptr), dev(indices), dev(seeds)
    for layer, local, n_dev in ((0, False, None), (1, True, len(seeds)), (1, False, len(seeds) - 3)):
        d_n = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device="cuda")
        src, dst, d_ne = hip.sample_khop_shared(d_indptr, d_indices, d_seeds, k, SEED, 9, layer,
                                                hip.SRC_LOCAL if local else hip.SRC_GLOBAL, d_num_input=d_n)
        want_src, want_dst = refs.sample(indptr, indices, seeds[:n_dev], k, SEED, 9, layer, src_local=local)
        ne = int(d_ne.cpu()[0])
        assert ne == len(want_dst)
        np.testing.assert_array_equal(u32(dst, ne), want_dst)
        np.testing.assert_array_equal(u32(src, ne), want_src)
    assert (u32(d_indices) == indices).all()  # the CSR is not touched


def test_more_hubs_than_the_list_holds_and_more_tiles_than_one_pass():
    """16500 copies of a hub seed: those beyond the hub list are selected by their owners from the row itself.  Then
    more than kSinglePassMaxTiles (1536) tiles of 256 one-entry rows: count, scan, emit."""
    block = hip.khop_shared_params()["block_row"]
    rng = np.random.default_rng(3)
    indptr, indices = _graph([rng.integers(0, NUM_NODE, block + 1)], NUM_NODE)
    one_src, one_dst = refs.sample(indptr, indices, [0], 25, SEED, 4, 0)
    ws = torch.empty(hip.load().fgnn_khop_shared_scratch_bytes(16500, 25), dtype=torch.uint8, device="cuda")
    src, dst, d_ne = hip.sample_khop_shared(dev(indptr), dev(indices), dev(np.zeros(16500, np.uint32)), 25, SEED, 4, 0,
                                            ws=ws)
    assert int(d_ne.cpu()[0]) == 16500 * 25
    pool = hip.khop_shared_pool_params()
    state = hip.debug_khop_shared_hub_state(ws, 16500)  # the list was too short, the pool was not
    assert state["count"] == 16500 > pool["max_hubs"]
    assert state["used"] == state["end"] == pool["max_hubs"] * 2 * 25 < pool["hub_pool"]
    np.testing.assert_array_equal(u32(dst, 16500 * 25), np.tile(one_dst, 16500))
    np.testing.assert_array_equal(u32(src, 16500 * 25), np.tile(one_src, 16500))

    n = 1536 * 256 + 5
    indptr = np.arange(1001, dtype=np.uint32)
    indices = rng.permutation(1000).astype(np.uint32)
    seeds = rng.integers(0, 1000, n).astype(np.uint32)
    src, dst, d_ne = hip.sample_khop_shared(dev(indptr), dev(indices), dev(seeds), 5, SEED, 4, 0, hip.SRC_LOCAL)
    assert int(d_ne.cpu()[0]) == n
    np.testing.assert_array_equal(u32(dst, n), indices[seeds])
    np.testing.assert_array_equal(u32(src, n), np.arange(n, dtype=np.uint32))


def _hub_rows_as_seeds(rows, seeds, fanout, key):
    """the stateless entry point over `seeds` (indices into the few distinct `rows`) with a scratch buffer of the test's
    own; the reference is computed once per distinct row and tiled.  Returns the hub scan's read-back."""
    indptr, indices = _graph(rows, NUM_NODE)
    one_src, one_dst = refs.sample(indptr, indices, np.arange(len(rows)), fanout, SEED, key, 0)
    assert len(one_dst) == len(rows) * fanout
    ws = torch.empty(hip.load().fgnn_khop_shared_scratch_bytes(len(seeds), fanout), dtype=torch.uint8, device="cuda")
    src, dst, d_ne = hip.sample_khop_shared(dev(indptr), dev(indices), dev(seeds), fanout, SEED, key, 0, ws=ws)
    ne = len(seeds) * fanout
    assert int(d_ne.cpu()[0]) == ne
    np.testing.assert_array_equal(u32(dst, ne), one_dst.reshape(len(rows), fanout)[seeds].reshape(-1))
    np.testing.assert_array_equal(u32(src, ne), np.repeat(seeds, fanout))
    return hip.debug_khop_shared_hub_state(ws, len(seeds))


def test_hubs_that_find_no_room_in_the_pool_while_the_list_has_room():
    """Fewer hubs than the list holds, whose claims together exceed the candidate pool: the hubs that claim first get their
    pieces reduced by the whole chip, the others (which ones is a race) are streamed by their owners.  The read-back
    shows that both happened in this run.  Fanout at the limit; rows of 65, 40 and 3 pieces, the last one of five ids
    only, so that its ties cross the pieces."""
    p, pool = hip.khop_shared_params(), hip.khop_shared_pool_params()
    k, block = p["max_fanout"], p["block_row"]
    rng = np.random.default_rng(31)
    pieces = np.array([65, 40, 3])
    rows = [rng.integers(0, NUM_NODE, 64 * block + 100), rng.integers(0, NUM_NODE, 39 * block + 1),
            rng.choice([5, 6, 7, 8, 9], 2 * block + 100)]
    assert [(len(r) - 1) // block + 1 for r in rows] == pieces.tolist()
    seeds = rng.permutation(np.repeat([0, 1, 2], [700, 500, 300])).astype(np.uint32)
    claims = int((pieces[seeds] * k).sum())
    assert len(seeds) < pool["max_hubs"] and claims > pool["hub_pool"]
    state = _hub_rows_as_seeds(rows, seeds, k, 6)
    assert state["count"] == len(seeds) and state["used"] == claims
    assert 0 < state["end"] <= pool["hub_pool"]  # some hubs had room; those claiming beyond the end had none
    assert state["end"] % k == 0 and state["end"] >= pool["hub_pool"] - 65 * k  # the pool filled up to its last claim


def test_claims_that_fill_the_pool_and_the_list_exactly():
    """as many hubs as the list holds, each of four pieces: the last claim ends on the pool's last pair and all have room"""
    p, pool = hip.khop_shared_params(), hip.khop_shared_pool_params()
    k, block = p["max_fanout"], p["block_row"]
    per_hub = pool["hub_pool"] // pool["max_hubs"]
    assert per_hub * pool["max_hubs"] == pool["hub_pool"] and per_hub % k == 0
    rows = [np.random.default_rng(32).integers(0, NUM_NODE, (per_hub // k - 1) * block + 5)]
    state = _hub_rows_as_seeds(rows, np.zeros(pool["max_hubs"], np.uint32), k, 7)
    assert state == dict(count=pool["max_hubs"], end=pool["hub_pool"], used=pool["hub_pool"])


def test_seeds_with_the_same_row_share_their_picks():
    row = np.random.default_rng(5).permutation(NUM_NODE)[:1000]
    indptr, indices = _graph([row, row], NUM_NODE)
    d = dev(indptr), dev(indices), dev(np.array([0, 1], np.uint32))
    picks = {}
    for key, layer in ((1, 0), (1, 1), (2, 0)):
        src, dst, d_ne = hip.sample_khop_shared(*d, 10, SEED, key, layer)
        got = u32(dst, 20)
        assert int(d_ne.cpu()[0]) == 20 and (got[:10] == got[10:]).all()
        picks[key, layer] = got[:10].tolist()
    assert picks[1, 0] != picks[1, 1] and picks[1, 0] != picks[2, 0]  # fresh keys per layer and per batch


@pytest.fixture(scope="module")
def hubby():
    # 2000 nodes, 16 random neighbours each, and three hubs (one beyond the workgroup's row length)
    rng = np.random.default_rng(11)
    rows = [rng.integers(0, 2000, 16) for _ in range(2000)]
    for node, n in ((3, 1500), (700, 9000), (1999, 5000)):
        rows[node] = rng.integers(0, 2000, n)
        for r in rows[::7]:
            r[0] = node  # the hubs are in many frontiers
    return _graph(rows, 2000)


def test_batch_driver(hubby):
    indptr, indices = hubby
    fanouts, rng = [5, 3], np.random.default_rng(12)
    sampler = hip.Sampler(dev(indptr), dev(indices), fanouts, 300, sample_type=hip.KHOP_SHARED, seed=SEED)
    feat, label = dev(np.zeros((2000, 4), np.float32)), dev(np.arange(2000, dtype=np.int64))
    seeds = [rng.permutation(2000)[:n].astype(np.uint32) for n in (300, 177, 300)]
    batches = [sampler.new_batch(4, hip.F32, hip.I64) for _ in seeds]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in (0, 1):  # two batches in flight on two streams
        with torch.cuda.stream(streams[i]):
            sampler.sample(dev(seeds[i]), 40 + i, batches[i], seq=i)
            batches[i].finish()
    sampler.run_batch(2, dev(seeds[2]), 42, batches[2], None, feat, label)
    for i, bt in enumerate(batches):
        assert bt.wait().overflow == 0
        graphs = [tuple(u32(x) if k < 2 else x for k, x in enumerate(bt.graph(l))) for l in (0, 1)]
        refs.check_batch(indptr, indices, u32(bt.input_nodes()), graphs, fanouts, seeds[i], SEED, 40 + i)
    np.testing.assert_array_equal(batches[2].label().cpu().numpy(), seeds[2])


def test_refusals_launch_nothing(hubby):
    L, p = hip.load(), hip._ptr
    indptr, indices = dev(hubby[0]), dev(hubby[1])
    inp = dev(np.array([3, 4], np.uint32))
    limit = hip.khop_shared_params()["max_fanout"]
    need = L.fgnn_khop_shared_scratch_bytes(2, 5)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = [torch.full((2 * (limit + 1),), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_ne = torch.full((1,), -1, dtype=torch.int64, device="cuda")

    def call(fanout=5, ws_bytes=need, indptr=indptr):
        return L.fgnn_sample_khop_shared(p(indptr), p(indices), p(inp), 2, None, 2, fanout, p(out[0]), p(out[1]), p(d_ne),
                                         hip.SRC_GLOBAL, SEED, 1, 0, p(ws), ws_bytes, hip._stream())
    assert call(fanout=0) == -1 and call(fanout=limit + 1) == -1 and call(indptr=None) == -1
    assert call(ws_bytes=need - 1) == -2
    torch.cuda.synchronize()
    assert int(d_ne.cpu()[0]) == -1 and all((o == -1).all() for o in out)
    assert call() == 0 and int(d_ne.cpu()[0]) == 10


def test_engine_arch1(tmp_path):
    """arch1 batches of the engine with sample type khop_shared, in a process of their own"""
    runner = os.path.join(os.path.dirname(os.path.abspath(__file__)), "khop_shared_engine_runner.py")
    r = subprocess.run([sys.executable, runner, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "khop_shared arch1 ok" in r.stdout, r.stdout[-3000:] + "\n" + r.stderr[-6000:]
