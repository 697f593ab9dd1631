"""What the samplers and the batch driver REFUSE, and what they do with an empty frontier: the return code of every
argument check in the launchers of sample_khop.hip, sample_weighted.hip, sample_hash_dedup.hip, sample_random_walk.hip
and in fgnn_sampler_create / the batch driver's entry points (engine.hip).

Every call here is either refused on the host before anything is launched, or is an empty call (a zeroed count word, no
kernel): nothing reaches a kernel with a bad pointer.  The k-hop launcher checks no pointer for null, so its cases pass
valid ones only.  The graph has 4 nodes, the frontier 2 seeds; scratch sizes are the library's own *_scratch_bytes."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, EINVAL, ENOSPC = 0, -1, -2
SEED, KEY, LAYER = 0x5A4D47, 3, 0
KHOP = ("khop0", "khop2")
WITH_REPLACEMENT = ("khop1", "weighted_khop", "weighted_khop_prefix")
ALL = KHOP + WITH_REPLACEMENT + ("weighted_khop_hash_dedup", "random_walk")


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


@pytest.fixture(scope="module")
def world(hip):
    """a 4-node ring with two neighbours per node, its weight tables, two seeds and room for every output"""
    def i32(a):
        return torch.tensor(a, dtype=torch.int32, device="cuda")
    L = hip.load()
    w = SimpleNamespace(indptr=i32([0, 2, 4, 6, 8]), indices=i32([1, 3, 0, 2, 1, 3, 0, 2]),
                        prob=torch.full((8,), 0.5, dtype=torch.float32, device="cuda"),
                        alias=i32([3, 1, 2, 0, 3, 1, 2, 0]),
                        prefix=torch.tensor([0.5, 1.0] * 4, dtype=torch.float32, device="cuda"),
                        input=i32([0, 2]), out_src=i32([0] * 64), out_dst=i32([0] * 64), out_data=i32([0] * 64),
                        d_num_out=torch.zeros(1, dtype=torch.int64, device="cuda"))
    w.ws_bytes = {"khop0": L.fgnn_scratch_bytes(2), "khop2": L.fgnn_scratch_bytes(2),
                  "khop1": L.fgnn_weighted_scratch_bytes(2, 2), "weighted_khop": L.fgnn_weighted_scratch_bytes(2, 2),
                  "weighted_khop_prefix": L.fgnn_weighted_scratch_bytes(2, 2),
                  "weighted_khop_hash_dedup": L.fgnn_hash_dedup_scratch_bytes(2),
                  "random_walk": L.fgnn_random_walk_scratch_bytes(2, 2)}
    w.ws = torch.empty(max(w.ws_bytes.values()), dtype=torch.uint8, device="cuda")
    return w


def _call(hip, w, kind, **change):
    """the stateless C entry point of `kind` on the world's valid arguments, with `change` applied; fanout is also the
    random walk's K.  Returns the code."""
    L, p = hip.load(), hip._ptr
    a = dict(indptr=w.indptr, indices=w.indices, prob=w.prob, alias=w.alias, prefix=w.prefix, input=w.input,
             num_input=2, fanout=2, out_src=w.out_src, out_dst=w.out_dst, out_data=w.out_data, d_num_out=w.d_num_out,
             ws=w.ws, ws_bytes=w.ws_bytes[kind], walk_len=2, num_walks=2)
    a.update(change)
    head = [p(a["indptr"]), p(a["indices"])]
    front = [p(a["input"]), a["num_input"], None, a["num_input"]]
    back = [p(a["d_num_out"]), hip.SRC_GLOBAL, SEED, KEY, LAYER, p(a["ws"]), a["ws_bytes"], hip._stream()]
    if kind == "random_walk":
        return L.fgnn_sample_random_walk(*head, *front, a["walk_len"], 0.5, a["num_walks"], a["fanout"],
                                         p(a["out_src"]), p(a["out_dst"]), p(a["out_data"]), *back)
    tables = {"weighted_khop_prefix": [p(a["prefix"])], "weighted_khop": [p(a["prob"]), p(a["alias"])],
              "weighted_khop_hash_dedup": [p(a["prob"]), p(a["alias"])]}.get(kind, [])
    fn = getattr(L, "fgnn_sample_" + kind)
    return fn(*head, *tables, *front, a["fanout"], p(a["out_src"]), p(a["out_dst"]), *back)


@pytest.mark.parametrize("kind", ALL)
def test_zero_fanout_is_refused(hip, world, kind):
    assert _call(hip, world, kind, fanout=0) == EINVAL


@pytest.mark.parametrize("kind", ALL)
def test_empty_frontier_zeroes_the_count(hip, world, kind):
    world.d_num_out.fill_(7)
    assert _call(hip, world, kind, num_input=0) == OK
    assert int(world.d_num_out.cpu()[0]) == 0


def test_khop_refusals(hip, world):
    assert _call(hip, world, "khop2", fanout=201) == EINVAL  # 3 * 201 * 64 words of LDS exceed 150 KiB
    assert _call(hip, world, "khop0", fanout=601) == EINVAL  # 601 * 64 words do
    for kind in KHOP:
        assert _call(hip, world, kind, ws_bytes=0) == ENOSPC


@pytest.mark.parametrize("kind", WITH_REPLACEMENT)
def test_with_replacement_refusals(hip, world, kind):
    assert _call(hip, world, kind, fanout=0x10000) == EINVAL
    for name in ("indptr", "indices", "input"):
        assert _call(hip, world, kind, **{name: None}) == EINVAL, name
    assert _call(hip, world, kind, ws_bytes=world.ws_bytes[kind] - 1) == ENOSPC


def test_weighted_samplers_need_their_tables(hip, world):
    assert _call(hip, world, "weighted_khop", alias=None) == EINVAL
    assert _call(hip, world, "weighted_khop_prefix", prefix=None) == EINVAL


def test_hash_dedup_refusals(hip, world):
    kind = "weighted_khop_hash_dedup"
    assert _call(hip, world, kind, fanout=51) == EINVAL  # the reference's 50-slot table
    assert _call(hip, world, kind, prob=None) == EINVAL
    assert _call(hip, world, kind, alias=None) == EINVAL
    assert _call(hip, world, kind, ws_bytes=8) == ENOSPC  # one descriptor and the ticket word take 16


def test_random_walk_refusals(hip, world):
    kind = "random_walk"
    assert _call(hip, world, kind, walk_len=0) == EINVAL
    assert _call(hip, world, kind, num_walks=0) == EINVAL
    assert _call(hip, world, kind, walk_len=4097, num_walks=1) == EINVAL  # more than 4096 steps per seed
    assert _call(hip, world, kind, fanout=0x10000) == EINVAL
    assert _call(hip, world, kind, out_data=None) == EINVAL
    assert _call(hip, world, kind, ws_bytes=world.ws_bytes[kind] - 1) == ENOSPC


def _config(hip, w, sample_type, fanout=(2,), max_batch_size=2, num_layers=None, **tables):
    cfg = hip.SamplerConfig()
    cfg.indptr, cfg.indices, cfg.num_node = w.indptr.data_ptr(), w.indices.data_ptr(), 4
    cfg.sample_type, cfg.num_layers = sample_type, len(fanout) if num_layers is None else num_layers
    for i, f in enumerate(fanout):
        cfg.fanout[i] = f
    cfg.max_batch_size, cfg.seed = max_batch_size, SEED
    for name, value in tables.items():
        setattr(cfg, name, value.data_ptr() if hasattr(value, "data_ptr") else value)
    return cfg


def test_sampler_create_refusals(hip, world):
    w = world
    both = dict(prob_table=w.prob, alias_table=w.alias)
    refused = {
        "zero layers": _config(hip, w, hip.KHOP0, fanout=()),
        "too many layers": _config(hip, w, hip.KHOP0, fanout=(2,) * hip.MAX_LAYERS, num_layers=hip.MAX_LAYERS + 1),
        "zero fanout": _config(hip, w, hip.KHOP0, fanout=(2, 0)),
        "zero batch size": _config(hip, w, hip.KHOP0, max_batch_size=0),
        "unknown sample type": _config(hip, w, 99),
        "weighted_khop without alias table": _config(hip, w, hip.WEIGHTED_KHOP, prob_table=w.prob),
        "weighted_khop without prob table": _config(hip, w, hip.WEIGHTED_KHOP, alias_table=w.alias),
        "hash_dedup without tables": _config(hip, w, hip.WEIGHTED_KHOP_HASH_DEDUP),
        "prefix without table": _config(hip, w, hip.WEIGHTED_KHOP_PREFIX),
        "hash_dedup fanout 51": _config(hip, w, hip.WEIGHTED_KHOP_HASH_DEDUP, fanout=(51,), **both),
        "random walk without steps": _config(hip, w, hip.RANDOM_WALK, walk_len=0, num_walks=2),
    }
    L = hip.load()
    for what, cfg in refused.items():
        err = C.c_int(5)
        assert not L.fgnn_sampler_create(C.byref(cfg), C.byref(err)), what
        assert err.value == EINVAL, what


def test_batch_driver_refusals(hip, world):
    L, w, st = hip.load(), world, hip._stream()
    mine = hip.Sampler(w.indptr, w.indices, [2], 2, sample_type=hip.KHOP0, seed=SEED)
    other = hip.Sampler(w.indptr, w.indices, [2], 2, sample_type=hip.KHOP0, seed=SEED)
    bt, foreign = mine.new_batch(), other.new_batch()
    three = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    # the _ordered entry points: a refusal there has taken no sequence number (the unordered one takes its number first,
    # and the calls after a refused one would wait for it); both samplers are destroyed when this function returns
    assert L.fgnn_sampler_sample_ordered(mine.h, 0, three.data_ptr(), 3, KEY, bt.h, st) == EINVAL
    assert L.fgnn_sampler_sample_ordered(mine.h, 0, w.input.data_ptr(), 2, KEY, foreign.h, st) == EINVAL
    assert L.fgnn_sampler_sample_begin_ordered(mine.h, 0, w.input.data_ptr(), 2, KEY, foreign.h, st) == EINVAL
    assert L.fgnn_sampler_sample_end(mine.h, 0, bt.h, None, st) == EINVAL  # no chain of batch 0 is pending
