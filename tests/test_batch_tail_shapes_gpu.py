"""The per-batch launch shapes of the batch driver change no result.

A batch that comes in through fgnn_sampler_run_batch / fgnn_sampler_run_range WITH a feature source is known to have a
bandwidth-bound feature gather beside its dedup launches on the same GPU, and the partitioned fill then runs its
histogram / scatter launches as 256-thread workgroups (engine.hip: ChainState::gather_follows, hashtable_partition.hip:
partition_fill); every other entry point keeps the 1024-thread shapes.  Both must produce the same bytes.

Each case runs EIGHT consecutive batches (the CSR state khop2 mutates and the dedup tables' generations carry over)
through two samplers of the same seed over their own copies of the CSR:
  * set path:    run_batch(..., table, feat, label)                      [or run_range, three streams / six buffers]
  * unset path:  sample_indexed(..., table); extract(feat, label); finish
and compares, bit for bit, everything a caller receives: row / col / counts per layer, input and output nodes, the four
cache-index arrays with num_miss / num_cache, labels and features.

Shapes: a 20 000-node R-MAT graph; fanout [25, 10] and a one-layer [3]; batch sizes 1, 64, an empty batch and three
sizes found by probing so that the last fill's item space (known nodes + the layer's edges, what the 4096-item
partition tiles are cut from) lands just under one tile, just over one and just over two; cache tables all -1, all
cached and every third node.  With khop2 a one-layer batch inserts in the sampler launch and never reaches the
partitioned fill, so the one-layer shape also runs with khop1, whose every fill is partitioned, at sizes probed in the
same way.

One case runs a 400 000-node graph at batch 16 000: its last fill holds more than 2^19 items, i.e. more than 256 bins,
where a 256-thread workgroup owns several bins per thread (the papers100M shape has exactly 256).

One case runs with the single-pass kernels' helping path forced (fgnn_debug_set_scan_help_after(0), as
test_scan_wrap_gpu.py does)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x5A4D47
NUM_NODE, NUM_EDGE, DIM = 20000, 300000, 32
TILE = 4096


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    assert lib.debug_partition_params()["tile"] == TILE
    return lib


@pytest.fixture(scope="module")
def world(hip):
    from fgnn_hip import rmat
    dev = torch.device("cuda", 0)
    indptr, indices, _ = rmat.rmat_csr(NUM_NODE, NUM_EDGE, seed=42, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    feat = torch.rand((NUM_NODE, DIM), generator=g, device=dev, dtype=torch.float32)
    label = torch.randint(0, 47, (NUM_NODE,), generator=g, device=dev, dtype=torch.int64)
    deg = (indptr[1:] - indptr[:-1]).to(torch.int64)
    perm = torch.randperm(NUM_NODE, generator=g, device=dev)
    perm = perm[deg[perm] >= 3].to(torch.int32).contiguous()  # (khop1: exactly 3 edges per seed)
    assert perm.numel() >= 2304
    ids = torch.arange(NUM_NODE, device=dev, dtype=torch.int32)
    tables = {"none": torch.full((NUM_NODE,), -1, dtype=torch.int32, device=dev),
              "all": ids.clone(),
              "third": torch.where(ids % 3 == 0, ids // 3, torch.full_like(ids, -1))}
    torch.cuda.synchronize()
    return dict(dev=dev, indptr=indptr, indices=indices, feat=feat, label=label, perm=perm, tables=tables)


def _seeds(world, k, n):
    """batch k's seeds: n distinct ids, a run of the (cyclic) seed list that starts at the batch's own offset"""
    perm = world["perm"]
    at = (k * 977 + torch.arange(n, device=perm.device)) % perm.numel()
    return perm[at].contiguous()


def _sampler(hip, world, fanout, kind, max_batch):
    idx = world["indices"].clone()  # khop2 swaps entries in place: every sampler owns its CSR
    torch.cuda.synchronize()
    s = hip.Sampler(world["indptr"], idx, fanout, max_batch, sample_type=kind, seed=SEED)
    s.csr_indices = idx
    return s


def _last_fill_items(m):
    return int(m.num_dst[0]) + int(m.num_edge[0])


def _tile_sizes(hip, world, fanout, kind, largest):
    """batch sizes whose last fill lands just under one partition tile (with batch 0's seeds and key), just over one
    (batch 1's) and just over two (batch 2's): bisection over the batch size, each probe a fresh sampler"""
    def items(k, n):
        s = _sampler(hip, world, fanout, kind, largest)
        bt = s.new_batch(0, hip.F32, hip.I64)
        s.sample_indexed(_seeds(world, k, n), k, bt, None)
        bt.finish()
        return _last_fill_items(bt.wait())

    def smallest_reaching(k, want):
        lo, hi = 1, largest
        assert items(k, hi) >= want
        while lo < hi:
            mid = (lo + hi) // 2
            if items(k, mid) >= want:
                hi = mid
            else:
                lo = mid + 1
        return lo

    under = smallest_reaching(0, int(TILE * 0.97)) - 1
    over1 = smallest_reaching(1, int(TILE * 1.03))
    over2 = smallest_reaching(2, int(2 * TILE * 1.03))
    assert 1 <= under < over2 <= largest
    return under, over1, over2


@pytest.fixture(scope="module")
def tile_sizes(hip, world):
    return _tile_sizes(hip, world, [25, 10], hip.KHOP2, 256)


def _snapshot(bt, m, num_layers, with_feat=True):
    """everything the caller receives from a waited-for batch, as CPU tensors"""
    out = {"counts": (int(m.num_input), int(m.num_output), int(m.num_miss), int(m.num_cache), int(m.overflow)),
           "input": bt.input_nodes().cpu(), "output": bt.output_nodes().cpu()}
    for k, a in enumerate(bt.cache_index_arrays()):
        out["cidx%d" % k] = a.cpu()
    for l in range(num_layers):
        row, col, nsrc, ndst = bt.graph(l)
        out["row%d" % l], out["col%d" % l] = row.cpu(), col.cpu()
        out["layer%d" % l] = (int(m.num_edge[l]), nsrc, ndst)
    if with_feat:
        out["feat"], out["label"] = bt.feat().cpu(), bt.label().cpu()
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], tuple):
            assert a[k] == b[k], (what, k, a[k], b[k])
        else:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def _unset_path(hip, world, sampler, bt, seeds, key, table):
    sampler.sample_indexed(seeds, key, bt, table)
    bt.extract(world["feat"], world["label"])
    bt.finish()
    return bt.wait()


def _compare_sequence(hip, world, fanout, kind, sizes, table):
    a = _sampler(hip, world, fanout, kind, max(sizes))
    b = _sampler(hip, world, fanout, kind, max(sizes))
    bta, btb = a.new_batch(DIM, hip.F32, hip.I64), b.new_batch(DIM, hip.F32, hip.I64)
    metas = []
    for k, n in enumerate(sizes):
        seeds = _seeds(world, k, n)
        a.run_batch(k, seeds, k, bta, table, world["feat"], world["label"])
        ma = bta.wait()
        mb = _unset_path(hip, world, b, btb, seeds, k, table)
        assert ma.overflow == 0 and int(ma.num_output) == n
        _same(_snapshot(bta, ma, len(fanout)), _snapshot(btb, mb, len(fanout)), "batch %d of %d seeds" % (k, n))
        metas.append(ma)
    assert torch.equal(a.csr_indices, b.csr_indices)  # the CSR the two samplers leave behind
    return metas


@pytest.mark.parametrize("table", ["third", "none", "all"])
def test_two_layers_around_the_tile_boundaries(hip, world, tile_sizes, table):
    under, over1, over2 = tile_sizes
    sizes = [under, over1, over2, 1, 64, 0, over1, under]
    metas = _compare_sequence(hip, world, [25, 10], hip.KHOP2, sizes, world["tables"][table])
    got = [_last_fill_items(m) for m in metas]
    print("batch sizes", sizes, "items of the last fill", got)
    assert got[0] <= TILE < got[1] <= 2 * TILE < got[2], (sizes, got)
    assert got[5] == 0 and int(metas[5].num_input) == 0
    if table != "third":
        assert all(int(m.num_miss if table == "all" else m.num_cache) == 0 for m in metas)


def test_one_layer_khop2(hip, world):
    _compare_sequence(hip, world, [3], hip.KHOP2, [1023, 1025, 2049, 1, 64, 0, 1025, 1023], world["tables"]["third"])


def test_one_layer_khop1(hip, world):
    """every fill of a khop1 batch is partitioned, the one of a one-layer batch too"""
    under, over1, over2 = _tile_sizes(hip, world, [3], hip.KHOP1, 2304)
    sizes = [under, over1, over2, 1, 64, 0, over1, under]
    metas = _compare_sequence(hip, world, [3], hip.KHOP1, sizes, world["tables"]["third"])
    got = [_last_fill_items(m) for m in metas]
    print("batch sizes", sizes, "items of the last fill", got)
    assert got[0] <= TILE < got[1] <= 2 * TILE < got[2], (sizes, got)


def test_more_bins_than_threads(hip):
    """a last fill of more than 256 x 2048 items: 512 bins or more, several per thread of a 256-thread workgroup"""
    from fgnn_hip import rmat
    dev = torch.device("cuda", 0)
    n_node = 400000
    indptr, indices, _ = rmat.rmat_csr(n_node, 8000000, seed=7, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    ids = torch.arange(n_node, device=dev, dtype=torch.int32)
    big = dict(dev=dev, indptr=indptr, indices=indices, perm=torch.randperm(n_node, generator=g, device=dev).to(torch.int32),
               feat=torch.rand((n_node, DIM), generator=g, device=dev, dtype=torch.float32),
               label=torch.randint(0, 47, (n_node,), generator=g, device=dev, dtype=torch.int64))
    table = torch.where(ids % 3 == 0, ids // 3, torch.full_like(ids, -1))
    metas = _compare_sequence(hip, big, [25, 10], hip.KHOP2, [16000, 16000, 7000], table)
    got = [_last_fill_items(m) for m in metas]
    print("items of the last fill", got)
    assert got[0] > 256 * 2048 and got[1] > 256 * 2048, got


def test_helping_path_forced(hip, world, tile_sizes):
    under, over1, over2 = tile_sizes
    try:
        hip.load().fgnn_debug_set_scan_help_after(0)
        _compare_sequence(hip, world, [25, 10], hip.KHOP2, [over2, under, 64, 0, 1, over1, over2, 64],
                          world["tables"]["third"])
    finally:
        hip.load().fgnn_debug_set_scan_help_after(int(os.environ.get("FGNN_SCAN_HELP_AFTER", -1)))


def test_run_range_three_streams_six_buffers(hip, world, tile_sizes):
    """the native batch loop: eight batches (the last one short) over three streams and six buffers, with a feature
    source; the six batches its buffers still hold are compared in full, the two earlier ones by their summaries"""
    bs = tile_sizes[2]
    fanout, table, dev = [25, 10], world["tables"]["third"], world["dev"]
    train = world["perm"][:7 * bs + bs // 2].contiguous()
    a = _sampler(hip, world, fanout, hip.KHOP2, bs)
    b = _sampler(hip, world, fanout, hip.KHOP2, bs)
    batches = [a.new_batch(DIM, hip.F32, hip.I64) for _ in range(6)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    metas, _, _ = a.run_range(0, 8, train, bs, batches, streams, cache_table=table, feat=world["feat"],
                              label=world["label"])
    btb = b.new_batch(DIM, hip.F32, hip.I64)
    for i in range(8):
        mb = _unset_path(hip, world, b, btb, train[i * bs:(i + 1) * bs], i, table)
        want = _snapshot(btb, mb, 2)
        if i >= 2:
            bt = batches[i % 6]
            bt.meta = metas[i]
            _same(_snapshot(bt, metas[i], 2), want, "batch %d" % i)
        else:
            ma = metas[i]
            assert (int(ma.num_input), int(ma.num_output), int(ma.num_miss), int(ma.num_cache), 0) == want["counts"]
            for l in range(2):
                assert (int(ma.num_edge[l]), int(ma.num_src[l]), int(ma.num_dst[l])) == want["layer%d" % l]
    assert int(metas[7].num_output) == bs // 2
    assert torch.equal(a.csr_indices, b.csr_indices)
