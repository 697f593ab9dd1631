"""The single-pass prefix across workgroups (fgnn_device.h: ScanWs / ScanWsHost) over the wrap-arounds of its two
counters that are never reset, and scan.hip's one-workgroup fallback scan on its own.

  * the launch GENERATION of a descriptor set counts up to 0x3FFFFFFE; the launch after that waits for the device, wipes
    the descriptors and starts again at 1 (ScanWsHost::next).  In production that is reached after 2^30 launches on one
    set; here fgnn_debug_scan_set puts every set of a sampler and of its batch buffers a few launches before it.
  * the TICKET counter of the hash-dedup sampler is a 32-bit device word bumped once per workgroup and mirrored on the
    host; tile = ticket - base must hold modulo 2^32.

Everything is bit-exact against the oracle (or numpy).  Every test shows through fgnn_debug_scan_get that its wrap took
place in that very run -- the wipe counter went up / the ticket word passed 2^32 -- and that afterwards no descriptor
carries a generation above the current one: a missing wipe would leave the previous cycle's tags (about 2^30) in the
descriptors that the small grids after the wrap never rewrite, whether or not a poll happened to hit one."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_coresidency_gpu import _digest
from test_hip_parity import SEED, _seeds, dev, host_u32

pytestmark = pytest.mark.gpu

NUM_SLOTS = 6           # engine.hip kSlots: batch `seq` runs on slot seq % 6
NUM_BATCHES = 48        # eight turns of every slot
TICKET_START = 2**32 - 3


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


@pytest.fixture(scope="module")
def world(oracle):
    """the with-replacement parity tests' graph (4000 nodes, 70 000 edges) with its weight tables and a cache table"""
    from fgnn_hip import synth
    num_node = 4000
    indptr, indices = synth.powerlaw_csr(num_node, 70000, seed=37)
    prob, alias = synth.alias_tables(indptr, indices)
    prefix = synth.prob_prefix_table(indptr, indices)
    table = oracle.cache_table_build(np.random.default_rng(9).permutation(num_node).astype(np.uint32), num_node // 4,
                                     num_node)
    return SimpleNamespace(num_node=num_node, indptr=indptr, indices=indices, prob=prob, alias=alias, prefix=prefix,
                           table=table)


def _make_sampler(hip, oracle, w, kind, fanouts, max_batch, d_indices):
    """(sampler, oracle sample type, oracle keywords) of a sampler kind"""
    d_indptr = dev(w.indptr)
    if kind in ("khop0", "khop1", "khop2"):
        hst, ost = dict(khop0=(hip.KHOP0, oracle.KHOP0), khop1=(hip.KHOP1, oracle.KHOP1),
                        khop2=(hip.KHOP2, oracle.KHOP2))[kind]
        return hip.Sampler(d_indptr, d_indices, fanouts, max_batch, sample_type=hst, seed=SEED), ost, {}
    if kind == "weighted_khop_prefix":
        return (hip.Sampler(d_indptr, d_indices, fanouts, max_batch, sample_type=hip.WEIGHTED_KHOP_PREFIX, seed=SEED,
                            prob_prefix=dev(w.prefix)), oracle.WEIGHTED_KHOP_PREFIX, dict(prob_prefix=w.prefix))
    if kind == "random_walk":
        return (hip.Sampler(d_indptr, d_indices, fanouts, max_batch, sample_type=hip.RANDOM_WALK, seed=SEED, walk_len=3,
                            num_walks=8, restart_prob=0.5), oracle.RANDOM_WALK,
                dict(walk_len=3, num_walks=8, num_neighbor=fanouts[0], restart_prob=0.5))
    assert kind == "weighted_khop_hash_dedup"
    return (hip.Sampler(d_indptr, d_indices, fanouts, max_batch, sample_type=hip.WEIGHTED_KHOP_HASH_DEDUP, seed=SEED,
                        prob_table=dev(w.prob), alias_table=dev(w.alias)), oracle.WEIGHTED_KHOP_HASH_DEDUP,
            dict(prob_prefix=w.prob, alias_table=w.alias))


def _check_batch(hip, oracle, w, bt, m, want, num_layers, what, with_data=False):
    assert m.overflow == 0, what
    for li in range(num_layers):
        row, col, nsrc, ndst = bt.graph(li)
        g = want["graphs"][li]
        assert (len(row), nsrc, ndst) == (g["num_edge"], g["num_src"], g["num_dst"]), (what, li)
        np.testing.assert_array_equal(host_u32(row), g["row"], err_msg="%s layer %d" % (what, li))
        np.testing.assert_array_equal(host_u32(col), g["col"], err_msg="%s layer %d" % (what, li))
        if with_data:
            np.testing.assert_array_equal(host_u32(bt.graph_data(li)), g["data"], err_msg="%s layer %d" % (what, li))
    nodes = host_u32(bt.input_nodes())
    np.testing.assert_array_equal(nodes, want["input_nodes"], err_msg=what)
    for got, ref in zip(bt.cache_index_arrays(), oracle.get_miss_cache_index(w.table, nodes)):
        np.testing.assert_array_equal(host_u32(got), ref, err_msg=what)
    assert m.num_miss + m.num_cache == m.num_input == len(nodes), what


def _assert_wrapped(states, gen_start, what):
    """every descriptor set went through the wipe, and nothing of the previous cycle is left in it"""
    for i, st in enumerate(states):
        assert st.wipes >= 1, "%s: descriptor set %d never reached the generation wrap (gen %#x)" % (what, i, st.gen)
        assert 1 <= st.gen < gen_start, (what, i, st.gen)
        assert st.max_desc_gen <= st.gen, \
            "%s: set %d holds a descriptor of generation %#x, current %#x" % (what, i, st.max_desc_gen, st.gen)


def _drive_across_generation_wrap(hip, oracle, w, kind, ticket=-1):
    """NUM_BATCHES batches of a two-layer sampler through fgnn_sampler_run_batch with a cache table, one batch buffer,
    every generation set six launches before the limit.  The first three batches have four times the seeds: their
    grids stamp descriptors that no later, smaller grid writes again."""
    gen_start = hip.SCAN_GEN_LIMIT - 5
    fanouts = [5, 5] if kind == "random_walk" else [7, 5]
    nseed, big = 300, 1200
    d_indices, o_indices = dev(w.indices.copy()), w.indices.copy()
    sampler, ost, okw = _make_sampler(hip, oracle, w, kind, fanouts, big, d_indices)
    bt = sampler.new_batch()
    hip.debug_scan_set(sampler, gen=gen_start, ticket=ticket)
    hip.debug_scan_set(bt, gen=gen_start)
    before = hip.debug_scan_states(sampler) + hip.debug_scan_states(bt)
    assert len(before) == 2 * NUM_SLOTS + 1
    assert all(st.gen == gen_start and st.wipes == 0 and st.max_desc_gen == 0 for st in before)
    if ticket >= 0:
        assert all(st.ticket_base == st.ticket_word == ticket for st in before[:-1])
    d_table = dev(w.table)
    oht = oracle.HashTable(w.num_node, sampler.max_nodes)
    rng = oracle.make_rng(oracle.RNG_PHILOX, SEED)
    for b in range(NUM_BATCHES):
        seeds = _seeds(big if b < 3 else nseed - b, w.num_node, seed=300 + b)
        sampler.run_batch(b, dev(seeds), 700 + b, bt, d_table)
        m = bt.wait()
        want = oracle.do_sample(w.indptr, o_indices, seeds, fanouts, ost, rng, 700 + b, oht, **okw)
        _check_batch(hip, oracle, w, bt, m, want, 2, "%s batch %d" % (kind, b), with_data=kind == "random_walk")
        if b == 2:
            # still the old cycle (no set has made six launches yet), and the large grids have stamped it
            mid = hip.debug_scan_states(sampler)[:2 * 3] + hip.debug_scan_states(bt)
            assert all(st.wipes == 0 and gen_start < st.max_desc_gen <= st.gen <= hip.SCAN_GEN_LIMIT for st in mid), \
                [(st.wipes, st.gen, st.max_desc_gen) for st in mid]
    if kind == "khop2":
        np.testing.assert_array_equal(host_u32(d_indices), o_indices)
    after = hip.debug_scan_states(sampler)
    _assert_wrapped(after + hip.debug_scan_states(bt), gen_start, kind)
    return after


def _forced_help(hip):
    """context: every wait of a single-pass kernel that its first poll does not satisfy takes the helping path"""
    class _Ctx:
        def __enter__(self):
            hip.load().fgnn_debug_set_scan_help_after(0)

        def __exit__(self, *exc):
            # back to what the session runs with (tests/conftest.py: FGNN_SCAN_HELP_AFTER, normally unset = default)
            hip.load().fgnn_debug_set_scan_help_after(int(os.environ.get("FGNN_SCAN_HELP_AFTER", -1)))
    return _Ctx()


@pytest.mark.parametrize("kind", ["khop0", "khop2", "khop1", "weighted_khop_prefix", "random_walk",
                                  "weighted_khop_hash_dedup"])
def test_batch_driver_across_the_scan_generation_wrap(hip, oracle, world, kind):
    """Per sampler family: the sampler's own single-pass launches (k-hop; seed-ranking prefix + emit of the
    with-replacement samplers; random walk; ticketed hash dedup), the dedup table's count+assign and the cache split
    all wrap their generation inside the run -- some between the two layers of one batch -- and every batch before, at
    and after it equals the oracle's."""
    _drive_across_generation_wrap(hip, oracle, world, kind)


@pytest.mark.parametrize("kind", ["khop2", "weighted_khop_prefix"])
def test_generation_wrap_with_the_helping_path_forced(hip, oracle, world, kind):
    """helpers publish on a missing tile's behalf (scan_prefix_help): what they stamp must be the new cycle's
    generation"""
    helps0 = int(hip.load().fgnn_debug_scan_helps())
    with _forced_help(hip):
        _drive_across_generation_wrap(hip, oracle, world, kind)
    print("helped tiles:", int(hip.load().fgnn_debug_scan_helps()) - helps0)


def test_generation_and_ticket_wrap_in_one_run(hip, oracle, world):
    """hash dedup: the ticket counters pass 2^32 in the slots' first batches, the generations wrap a few batches later"""
    after = _drive_across_generation_wrap(hip, oracle, world, "weighted_khop_hash_dedup", ticket=TICKET_START)
    for st in after[0::2]:  # the samplers' own sets (the tables' never draw tickets)
        assert st.ticket_base == st.ticket_word
        assert 8 <= st.ticket_word < 2**31, "the ticket counter did not pass 2^32: %#x" % st.ticket_word


def test_generation_wrap_with_batches_in_flight(hip, oracle, world):
    """fgnn_sampler_run_range over three streams and six buffers (the loop bench.py times): every set wraps inside the
    first native call, in batches 6..11, while other batches are in flight on the other streams -- the wipe must be
    fenced against them on both sides.  Against the same range run one batch at a time on one stream with untouched
    counters: summaries of all batches, contents of the batches each call leaves in the buffers, the final CSR."""
    w = world
    fanouts, bs, count, chunk = [7, 5], 400, 24, 12
    limit = hip.SCAN_GEN_LIMIT
    train = dev(_seeds(2400, w.num_node, seed=11))
    d_indptr, d_table = dev(w.indptr), dev(w.table)

    def run(n_streams, chunk, gens):
        d_indices = dev(w.indices.copy())
        sampler = hip.Sampler(d_indptr, d_indices, fanouts, bs, sample_type=hip.KHOP2, seed=SEED)
        batches = [sampler.new_batch() for _ in range(2 * n_streams)]
        streams = [torch.cuda.Stream() for _ in range(n_streams)]
        if gens:
            # two launches per slot and turn (sampler set, table's set), one per buffer and turn: all wrap in turn two
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
                assert all(st.gen <= 4 for st in states)  # ... and only just: in this call's second half
        torch.cuda.synchronize()
        return metas, digests, host_u32(d_indices)

    ref_metas, ref_digests, ref_csr = run(1, 1, gens=False)
    metas, digests, csr = run(3, chunk, gens=True)
    assert metas == ref_metas
    assert sorted(digests) == list(range(6, 12)) + list(range(18, 24))
    assert all(digests[i] == ref_digests[i] for i in digests), [i for i in digests if digests[i] != ref_digests[i]]
    np.testing.assert_array_equal(csr, ref_csr)


def _stateless_hash_dedup(hip, w, d, inp, fanout, batch_key, layer):
    """fgnn_sample_weighted_khop_hash_dedup with a scratch buffer of the test's own, to read the ticket word back: the
    stateless path keeps (workgroups) descriptors and then the counter in it, 8 bytes each"""
    L = hip.load()
    n = len(inp)
    nb = (n + 255) // 256
    d_inp = dev(inp)
    out_src = torch.empty(n * fanout, dtype=torch.int32, device="cuda")
    out_dst = torch.empty(n * fanout, dtype=torch.int32, device="cuda")
    d_ne = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(L.fgnn_hash_dedup_scratch_bytes(C.c_size_t(n)) // 8, dtype=torch.int64, device="cuda")
    assert ws.numel() >= nb + 1
    rc = L.fgnn_sample_weighted_khop_hash_dedup(
        C.c_void_p(d["indptr"].data_ptr()), C.c_void_p(d["indices"].data_ptr()), C.c_void_p(d["prob"].data_ptr()),
        C.c_void_p(d["alias"].data_ptr()), C.c_void_p(d_inp.data_ptr()), C.c_size_t(n), C.c_void_p(0), C.c_size_t(n),
        C.c_size_t(fanout), C.c_void_p(out_src.data_ptr()), C.c_void_p(out_dst.data_ptr()), C.c_void_p(d_ne.data_ptr()),
        C.c_int(hip.SRC_GLOBAL), C.c_uint64(SEED), C.c_uint64(batch_key), C.c_uint32(layer), C.c_void_p(ws.data_ptr()),
        C.c_size_t(ws.numel() * 8), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    ne = int(d_ne.cpu()[0])
    h_ws = ws.cpu().numpy().view(np.uint64)
    tags = (h_ws[:nb] >> np.uint64(34)).astype(np.int64)
    return host_u32(out_src, ne), host_u32(out_dst, ne), int(h_ws[nb] & np.uint64(0xFFFFFFFF)), nb, tags


@pytest.mark.parametrize("start", [2**32 - 3, 2**32 - 8, 2**32 - 9])
def test_stateless_hash_dedup_tickets_across_2_to_the_32(hip, oracle, world, start):
    """Nine workgroups draw their tiles from a counter that starts at `start`: tickets on both sides of zero; the last
    ticket exactly zero; the counter ending exactly at zero.  Then three launches more, started at zero again (the hook
    holds for one call)."""
    w = world
    d = dict(indptr=dev(w.indptr), indices=dev(w.indices), prob=dev(w.prob), alias=dev(w.alias))
    rng = oracle.make_rng(oracle.RNG_PHILOX, SEED)
    for call, n in enumerate([2100, 2100, 300, 2305]):
        inp = _seeds(n, w.num_node, seed=40 + call)
        if call == 0:
            hip.load().fgnn_debug_set_stateless_ticket_start_once(start)
        base = start if call == 0 else 0
        src, dst, word, nb, tags = _stateless_hash_dedup(hip, w, d, inp, 6, 50 + call, 1)
        o_src, o_dst = oracle.sample_weighted_khop_hash_dedup(w.indptr, w.indices, w.prob, w.alias, inp, 6, rng,
                                                              50 + call, 1)
        np.testing.assert_array_equal(src, o_src, err_msg="call %d" % call)
        np.testing.assert_array_equal(dst, o_dst, err_msg="call %d" % call)
        # every workgroup drew one ticket: the counter is where the host's base for a next launch would be
        assert word == (base + nb) % 2**32, (call, hex(word))
        assert (tags == 1).all()  # every tile published, with the stateless path's generation
        if call == 0:
            assert nb >= 8 and (word - start) % 2**32 == nb and start + nb >= 2**32  # the counter passed (reached) 2^32


def test_batch_driver_hash_dedup_tickets_across_2_to_the_32(hip, oracle, world):
    """every slot's counter (device word and host base) starts at 2^32 - 3; a slot's first launch has at least eight
    workgroups (one per 256 seeds), so its tickets straddle zero; two more turns of every slot follow.  After each batch
    base and word agree and have advanced by exactly the workgroups launched, modulo 2^32."""
    w = world
    fanouts, batch = [4, 3], 2100
    sampler, ost, okw = _make_sampler(hip, oracle, w, "weighted_khop_hash_dedup", fanouts, batch, dev(w.indices))
    bt = sampler.new_batch()
    hip.debug_scan_set(sampler, ticket=TICKET_START)
    assert all(st.ticket_base == st.ticket_word == TICKET_START for st in hip.debug_scan_states(sampler))
    d_table = dev(w.table)
    oht = oracle.HashTable(w.num_node, sampler.max_nodes)
    rng = oracle.make_rng(oracle.RNG_PHILOX, SEED)
    o_indices = w.indices.copy()
    drawn = [0] * NUM_SLOTS  # workgroups launched per slot: grids cover the worst case n and n * (1 + fanouts[1]) seeds
    for b in range(3 * NUM_SLOTS):
        n = batch - 7 * b
        seeds = _seeds(n, w.num_node, seed=500 + b)
        first, second = -(-n // 256), -(-n * (1 + fanouts[1]) // 256)
        assert first >= 8
        drawn[b % NUM_SLOTS] += first + second
        sampler.run_batch(b, dev(seeds), 40 + b, bt, d_table)
        m = bt.wait()
        want = oracle.do_sample(w.indptr, o_indices, seeds, fanouts, ost, rng, 40 + b, oht, **okw)
        _check_batch(hip, oracle, w, bt, m, want, 2, "batch %d" % b)
        for slot, st in enumerate(hip.debug_scan_states(sampler)[0::2]):
            assert st.ticket_base == st.ticket_word, (b, slot, hex(st.ticket_base), hex(st.ticket_word))
            assert st.ticket_word == (TICKET_START + drawn[slot]) % 2**32, (b, slot, hex(st.ticket_word))
            if slot <= b:  # used: past 2^32 since its first launch
                assert drawn[slot] >= 8 and st.ticket_word < 2**31, (b, slot)


# ---- scan.hip's one-workgroup scan on its own ----------------------------------------------------------------------
CANARY = 0xA5A5A5A5


def _scan(hip, sums, n=None, want_total64=True, want_total32=True, accum=None, same_word=False, accum_out=True,
          items32=None, items64=None, items_per_sum=0):
    """runs fgnn_debug_scan_block_sums on a copy of `sums` followed by 8 canary words; returns
    (scanned sums, canaries, total64, total32, accum_out, accum afterwards) -- None where not requested"""
    n = len(sums) if n is None else n
    buf = dev(np.concatenate([sums, np.full(8, CANARY, dtype=np.uint32)]).astype(np.uint32))
    t64 = torch.full((1,), -7, dtype=torch.int64, device="cuda") if want_total64 else None
    t32 = dev(np.array([CANARY], dtype=np.uint32)) if want_total32 else None
    d_acc = dev(np.array([accum], dtype=np.uint32)) if accum is not None else None
    d_out = None
    if accum_out:
        d_out = d_acc if same_word else dev(np.array([CANARY], dtype=np.uint32))
    d_i32 = dev(np.array([items32], dtype=np.uint32)) if items32 is not None else None
    d_i64 = torch.tensor([items64], dtype=torch.int64, device="cuda") if items64 is not None else None
    hip.debug_scan_block_sums(buf, n, total64=t64, total32=t32, accum=d_acc, accum_out=d_out, items32=d_i32,
                              items64=d_i64, items_per_sum=items_per_sum)
    out = host_u32(buf)
    one = lambda t: None if t is None else int(host_u32(t)[0])
    return (out[:len(sums)], out[len(sums):], None if t64 is None else int(t64.cpu()[0]), one(t32), one(d_out),
            one(d_acc))


def _reference(sums, live):
    """exclusive prefix sums of the first `live` entries modulo 2^32 (the rest untouched), and the total modulo 2^32"""
    live = min(live, len(sums))
    c = np.cumsum(sums[:live].astype(np.uint64), dtype=np.uint64)
    want = sums.copy()
    want[:live] = (np.concatenate([[0], c[:-1]]) % 2**32).astype(np.uint32) if live else []
    return want, (int(c[-1]) if live else 0)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2048, 3 * 1024 + 5, 200_000])
def test_scan_block_sums_matches_cumsum(hip, n):
    """whole rounds of the 1024-thread workgroup, one entry more and one less, a ragged tail, nothing at all"""
    rng = np.random.default_rng(n)
    sums = rng.integers(0, min(1 << 20, (2**32 - 1) // max(n, 1)) + 1, size=n, dtype=np.uint64).astype(np.uint32)
    want, total = _reference(sums, n)
    assert total < 2**32
    got, canary, t64, t32, acc_out, _ = _scan(hip, sums, accum=12345)
    np.testing.assert_array_equal(got, want)
    assert (canary == CANARY).all()
    assert (t64, t32, acc_out) == (total, total, (12345 + total) % 2**32)


def test_scan_block_sums_is_exact_modulo_2_to_the_32(hip):
    """a total beyond 2^32: prefixes, total32 and accum_out wrap; total64 is the wrapped total zero-extended, as
    fgnn_device.h documents (the arithmetic is 32-bit throughout)"""
    rng = np.random.default_rng(5)
    sums = rng.integers(0, 2**32, size=3 * 1024 + 5, dtype=np.uint64).astype(np.uint32)
    want, total = _reference(sums, len(sums))
    assert total > 2**32 * 1000
    got, canary, t64, t32, acc_out, _ = _scan(hip, sums, accum=0xFFFFFFF0)
    np.testing.assert_array_equal(got, want)
    assert (canary == CANARY).all()
    assert t32 == total % 2**32 and t64 == total % 2**32
    assert acc_out == (0xFFFFFFF0 + total) % 2**32


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("items_per_sum", [1, 64, 256])
@pytest.mark.parametrize("live", ["none", "below", "equal", "above"])
def test_scan_block_sums_clipped_by_a_device_item_count(hip, width, items_per_sum, live):
    """d_items32 / d_items64: only the first ceil(items / items_per_sum) entries are scanned and summed; the entries
    beyond come back untouched"""
    n = 3 * 1024 + 5
    rng = np.random.default_rng(items_per_sum + width)
    sums = rng.integers(1, 1 << 18, size=n, dtype=np.uint64).astype(np.uint32)
    # item counts that are no multiple of items_per_sum (where it is not 1): the last live entry is a partial one
    items = dict(none=0, below=items_per_sum * 1499 + 1, equal=items_per_sum * (n - 1) + 1,
                 above=items_per_sum * (n + 10))[live]
    n_live = -(-items // items_per_sum)
    assert dict(none=n_live == 0, below=n_live == 1500, equal=n_live == n, above=n_live > n)[live]
    want, total = _reference(sums, n_live)
    kw = dict(items32=items) if width == 32 else dict(items64=items)
    got, canary, t64, t32, acc_out, _ = _scan(hip, sums, accum=7, items_per_sum=items_per_sum, **kw)
    np.testing.assert_array_equal(got, want)
    assert (canary == CANARY).all()
    assert (t64, t32, acc_out) == (total, total, 7 + total)


def test_scan_block_sums_accumulator_and_optional_outputs(hip):
    """accum / accum_out as two words and as ONE word (how the dedup table advances its item count), accum_out without
    accum, no accum_out; total64 or total32 left out"""
    rng = np.random.default_rng(17)
    sums = rng.integers(0, 1 << 16, size=1025, dtype=np.uint64).astype(np.uint32)
    want, total = _reference(sums, len(sums))
    got, _, t64, t32, acc_out, acc = _scan(hip, sums, accum=1000)
    np.testing.assert_array_equal(got, want)
    assert (t64, t32, acc_out, acc) == (total, total, 1000 + total, 1000)  # the input word is only read
    got, _, t64, t32, acc_out, acc = _scan(hip, sums, accum=1000, same_word=True)
    np.testing.assert_array_equal(got, want)
    assert (t64, t32, acc_out, acc) == (total, total, 1000 + total, 1000 + total)
    got, _, t64, t32, acc_out, _ = _scan(hip, sums)  # accum_out without accum: the total
    np.testing.assert_array_equal(got, want)
    assert (t64, t32, acc_out) == (total, total, total)
    got, _, t64, t32, acc_out, acc = _scan(hip, sums, accum=1000, accum_out=False)
    np.testing.assert_array_equal(got, want)
    assert (t64, t32, acc_out, acc) == (total, total, None, 1000)
    got, _, t64, t32, _, _ = _scan(hip, sums, want_total64=False)
    np.testing.assert_array_equal(got, want)
    assert (t64, t32) == (None, total)
    got, _, t64, t32, _, _ = _scan(hip, sums, want_total32=False)
    np.testing.assert_array_equal(got, want)
    assert (t64, t32) == (total, None)
    got, _, t64, t32, acc_out, _ = _scan(hip, sums, want_total64=False, want_total32=False, accum_out=False)
    np.testing.assert_array_equal(got, want)  # nothing but the prefixes
