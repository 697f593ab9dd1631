"""GPU: the two dedup hash tables on node ids that collide -- long probe chains, chains across the end of the table, full
load, ids with the top bit set, live buckets among stale generations (csrc/hashtable.hip, the probes in
csrc/fgnn_device.h), and partition bins that are crowded, over the LDS limit, overflowing or hopeless
(csrc/hashtable_partition.hip).  The key sets and their regimes come from tests/ht_refs.py and are proven on the CPU by
tests/test_hashtable_adversarial_refs.py; the bar is bit-exact, against the plain first-occurrence reference (section A:
arbitrary 32-bit ids cannot go through the oracle's direct-indexed table) or oracle.do_sample (section B).

Which fills of section B run where (csrc/engine.hip): khop0 inserts from its sampler kernel, so every fill of it goes
through the GLOBAL table (fused insert; the resolving insert with take-over notes for the last of two layers); khop2's
last fill of a two-layer batch and every fill of khop1 (`table_free`) are PARTITIONED, and a bin that does not fit its
LDS table falls back to the global one."""
import numpy as np
import pytest
import torch

import ht_refs as R

pytestmark = pytest.mark.gpu


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host_u32(t, n=None):
    a = t.cpu().numpy()
    if n is not None:
        a = a[:n]
    return a.view(np.uint32) if a.dtype == np.int32 else a


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def test_library_constants_are_the_recorded_ones(hip):
    """every regime of this file is placed with tests/golden/partition_params.json: a changed constant fails here instead
    of silently moving a case out of its regime"""
    assert hip.debug_partition_params() == R.PARAMS
    for max_items in (512, 513, 1000, 2000, 10050):
        assert hip.HashTable(max_items).capacity() == R.table_capacity(max_items)


# ---- A: the stand-alone table through the C ABI ------------------------------------------------------------------------------

def _check_table(ht, known, items=None, mapped=None, want_mapped=None):
    assert ht.num_items() == len(known)
    np.testing.assert_array_equal(host_u32(ht.unique()), known)
    np.testing.assert_array_equal(host_u32(ht.map(dev(known))), np.arange(len(known), dtype=np.uint32))
    if items is not None:
        np.testing.assert_array_equal(host_u32(mapped, len(items)), want_mapped)
        np.testing.assert_array_equal(host_u32(ht.map(dev(items))), want_mapped)


def _run_steps(ht, steps):
    known = np.empty(0, dtype=np.uint32)
    for kind, ids in steps:
        if kind == "unique":
            ht.fill_unique(dev(ids))
            known = np.concatenate([known, ids])
            _check_table(ht, known)
        else:
            mapped = ht.fill_duplicates(dev(ids))
            known, want = R.first_occurrence_dedup(known, ids)
            _check_table(ht, known, ids, mapped, want)
    return known


@pytest.mark.parametrize("generations", [False, True])
@pytest.mark.parametrize("name", list(R.standalone_cases()))
def test_standalone_table_on_colliding_keys(hip, name, generations):
    """generations: max_fill_items given, so reset() is a generation bump and the table owns take-over notes and the
    partition scratch; else every reset wipes.  Twice around, so the second pass meets what the first left."""
    case = R.standalone_cases()[name]
    ht = hip.HashTable(case["max_items"], max_fill_items=4000 if generations else None)
    assert ht.capacity() == case["capacity"]
    for rep in range(2):
        ht.reset()
        final = _run_steps(ht, case["steps"])
        assert sorted(final) == sorted(case["keys"])


@pytest.mark.parametrize("max_fill", [None, (1 << 27) - 1])
def test_standalone_table_live_buckets_among_stale_ones(hip, max_fill):
    """20 resets over one 400-key single-home-slot chain, every generation another subset in another order: a live chain
    runs through buckets of earlier generations.  max_fill 2^27 - 1 leaves 3 generation bits: the 7th, 14th ... reset
    wipes, so generations either side of the physical wipe are included."""
    case = R.generation_case()
    ht = hip.HashTable(case["max_items"], max_fill_items=max_fill)
    assert ht.capacity() == case["capacity"]
    for uniq, items in case["gens"]:
        ht.reset()
        _run_steps(ht, [("unique", uniq), ("dup", items)])


# ---- B: the batch driver -------------------------------------------------------------------------------------------------------

def _run_sampler_case(hip, oracle, case, kind, name=None):
    """two batches through fgnn_sampler_sample on one sampler (the second finds table and partition scratch as the first
    left them) against the oracle; returns the oracle's results"""
    wants = []
    fills = R.sampler_regimes(oracle, case, kind, want_out=wants)
    if name is not None:
        R.check_regimes(name, case, fills)  # from the oracle's output: a case outside its regime fails, never passes idly
    d_indices = dev(case["indices"].copy())
    sampler = hip.Sampler(dev(case["indptr"]), d_indices, case["fanouts"], case["max_batch"],
                          sample_type=getattr(hip, kind), seed=0x5A4D47)
    assert sampler.max_nodes == R.predict_num_nodes(case["max_batch"], case["fanouts"])
    bt = sampler.new_batch()
    for b, (seeds, want) in enumerate(zip(case["batches"], wants)):
        sampler.sample(dev(seeds), 40 + b, bt)
        bt.finish()
        m = bt.wait()
        assert m.overflow == 0
        for li in range(len(case["fanouts"])):
            row, col, nsrc, ndst = bt.graph(li)
            g = want["graphs"][li]
            assert (len(row), nsrc, ndst) == (g["num_edge"], g["num_src"], g["num_dst"]), (b, li)
            np.testing.assert_array_equal(host_u32(row), g["row"])
            np.testing.assert_array_equal(host_u32(col), g["col"])
        np.testing.assert_array_equal(host_u32(bt.input_nodes()), want["input_nodes"])
    np.testing.assert_array_equal(host_u32(d_indices), case["indices"])
    for fb in fills:  # the figures the case was run at (pytest -s)
        print(name, kind, "total", fb["total"], "bins", 1 << fb["lg"],
              {bn: (int(fb["items"][bn]), int(fb["distinct"][bn]), fb["regime"][bn], fb["clusters"][bn])
               for bn in case["expect"]},
              "first fill", fb["first"] and (fb["first"]["total"], 1 << fb["first"]["lg"],
                                             sorted(set(fb["first"]["regime"]))))
    return wants


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("name", list(R.FLAT_CASES))
def test_batch_driver_on_crowded_partition_bins(hip, oracle, name, shape):
    """one_layer / khop0: the ids of the case through the fused insert into the global table; two_layers / khop2: through
    the partitioned last fill; unit_rows / khop1: both fills partitioned, the second the adversarial one"""
    _run_sampler_case(hip, oracle, R.sampler_case(name, shape), R.SAMPLER_KINDS[shape], name)


@pytest.mark.parametrize("name", R.CROSS_CASES)
def test_batch_driver_fall_back_in_one_fill_and_not_in_the_next(hip, oracle, name):
    """khop1, every fill partitioned: a bin of the first fill falls back and leaves its new keys pending in the global
    table; the last fill names all of them again, as known nodes, from a bin that falls back again (the pending values
    must lose against the local ids) or from LDS-resident bins (the table must not matter).  The reverse order is every
    fall-back case of test_batch_driver_on_crowded_partition_bins[*-unit_rows]."""
    _run_sampler_case(hip, oracle, R.cross_fill_case(name), "KHOP1", name)


@pytest.mark.parametrize("kind", ["KHOP0", "KHOP2"])
def test_batch_driver_on_colliding_global_slots(hip, oracle, kind):
    """mids and last-layer ids share 12 home slots either side of the end of the sampler's global table: the fused insert
    of the first-sampled layer, then khop0's resolving insert / khop2's partitioned fill of the last layer"""
    case = R.global_collision_case()
    assert hip.HashTable(case["max_nodes"]).capacity() == case["capacity"]
    wants = _run_sampler_case(hip, oracle, {**case, "expect": {}}, kind)
    for want in wants:
        length, wraps = R.global_collision_stats(case, want)
        print(kind, "longest global chain", length, "crosses the end", wraps)
        assert wraps and length >= 300
