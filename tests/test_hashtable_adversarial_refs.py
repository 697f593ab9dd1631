"""CPU-only: the constructions of tests/ht_refs.py have the hash properties, distinct-key counts and regimes that
tests/test_hashtable_adversarial_gpu.py relies on, and its plain reference agrees with a dict replay and with the oracle's
table.  Fails if a construction drifts (a changed seed, constant or hash mirror)."""
import numpy as np
import pytest

import ht_refs as R

P = R.PARAMS


def dict_replay(known, items):
    """the reference once more, as slowly and plainly as possible"""
    local = {}
    for k in known:
        assert int(k) not in local
        local[int(k)] = len(local)
    mapped = []
    for x in items:
        if int(x) not in local:
            local[int(x)] = len(local)
        mapped.append(local[int(x)])
    return np.array(list(local), dtype=np.uint32), np.array(mapped, dtype=np.uint32)


def test_hash_mirrors_and_the_inverse():
    assert (R.HASH_MULT * R.HASH_INV) % (1 << 32) == 1
    rng = np.random.default_rng(0)
    h = rng.integers(0, 1 << 32, size=5000, dtype=np.uint64)
    keys = R.keys_for_hashes(h)
    assert keys.dtype == np.uint32 and (R.hash32(keys) == h).all()
    for k in [0, 1, 12345, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE]:  # against plain Python integers
        hh = (k * 0x9E3779B1) & 0xFFFFFFFF
        assert int(R.global_slot([k], 1024)[0]) == (hh >> 22) & 1023
        assert int(R.global_slot([k], 1 << 17)[0]) == hh >> 15
        for lg in (5, 7, 11):
            assert int(R.part_bin([k], lg)[0]) == hh >> (32 - lg)
            assert int(R.part_slot([k], lg)[0]) == ((hh << lg) & 0xFFFFFFFF) >> 19
    assert [R.part_log2(t) for t in (0, 1, 65536, 65537, 131072, 131073, 1 << 30)] == [5, 5, 5, 6, 6, 7, 11]
    assert R.part_log2(1 << 20, 7) == 7 and R.table_capacity(512) == 1024 and R.table_capacity(513) == 2048
    assert (P["lds_slots"], P["lds_limit"], P["reg_items"], P["hopeless_items"], P["tile"]) == (8192, 6144, 4096, 32768,
                                                                                              4096)


def test_the_counts_the_constructions_rest_on():
    # 2000 distinct keys with home slot 1023 of a 1024-slot table exist, none of them the empty key
    keys = R.keys_with_homes(np.full(2000, 1023), 1024, np.random.default_rng(1))
    assert len(np.unique(keys)) == 2000 and (R.global_slot(keys, 1024) == 1023).all() and (keys != R.EMPTY).all()
    per_bin = np.bincount(R.part_bin(np.arange(R.NUM_NODE), 5), minlength=32)
    assert per_bin.min() > 131000 and per_bin.max() < 131150
    ids = R.ids_in_bin(R.BIN_A)
    per_slot = np.bincount(R.part_slot(ids, 5), minlength=P["lds_slots"])
    assert 13 <= per_slot.min() and per_slot.max() <= 18
    assert per_slot[-8:].sum() >= 120
    per_global = np.bincount(R.global_slot(np.arange(R.NUM_NODE), 1 << 17), minlength=1 << 17)
    assert 29 <= per_global.min() and per_global.max() <= 35


@pytest.mark.parametrize("seed", range(4))
def test_reference_agrees_with_a_dict_replay(seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 32, size=700, dtype=np.uint64).astype(np.uint32)
    pool = np.unique(np.concatenate([pool, [0, 0x80000000, 0xFFFFFFFE]]).astype(np.uint32))
    known = rng.permutation(pool)[:rng.integers(0, 200)]
    items = rng.choice(pool, size=3000)
    for k, it in ((known, items), (known[:0], items), (known, items[:0])):
        u, m = R.first_occurrence_dedup(k, it)
        u2, m2 = dict_replay(k, it)
        np.testing.assert_array_equal(u, u2)
        np.testing.assert_array_equal(m, m2)


def _replay_case(steps):
    known = np.empty(0, dtype=np.uint32)
    for kind, ids in steps:
        if kind == "unique":
            assert len(np.unique(ids)) == len(ids) and not np.isin(ids, known).any()
            known = np.concatenate([known, ids])
        else:
            u, m = R.first_occurrence_dedup(known, ids)
            u2, m2 = dict_replay(known, ids)
            np.testing.assert_array_equal(u, u2)
            np.testing.assert_array_equal(m, m2)
            known = u
    return known


def test_standalone_cases_have_their_properties():
    cases = R.standalone_cases()
    assert set(cases) == {"one_home_slot", "wrap_around", "load_half_random", "load_half_crowded", "load_just_over_random",
                          "load_just_over_crowded", "id_range", "interleaved_clusters"}
    for name, c in cases.items():
        keys, cap = c["keys"], c["capacity"]
        assert cap == R.table_capacity(c["max_items"])
        assert len(np.unique(keys)) == len(keys) <= c["max_items"] and (keys != R.EMPTY).all()
        final = _replay_case(c["steps"])
        assert sorted(final) == sorted(keys), name  # every key of the set is inserted, nothing else
        assert all(len(ids) <= 4000 for _, ids in c["steps"])
    homes = {n: R.global_slot(c["keys"], c["capacity"]) for n, c in cases.items()}
    assert len(cases["one_home_slot"]["keys"]) == 600 and (homes["one_home_slot"] == 1023).all()
    assert R.longest_cluster(homes["one_home_slot"], 2048) == (600, False)
    w = homes["wrap_around"]
    assert len(w) == 600 and w.min() >= 2048 - 8 and len(np.unique(w)) == 8
    length, wraps = R.longest_cluster(w, 2048)
    assert wraps and w.max() + length > 2048
    for n, n_keys, cap in (("load_half_random", 512, 1024), ("load_half_crowded", 512, 1024),
                           ("load_just_over_random", 513, 2048), ("load_just_over_crowded", 513, 2048)):
        assert len(cases[n]["keys"]) == n_keys and cases[n]["capacity"] == cap
        if "crowded" in n:
            assert len(np.unique(homes[n])) == 16 and R.longest_cluster(homes[n], cap) == (n_keys, True)
        else:
            assert (cases[n]["keys"] >= 1 << 31).sum() > n_keys // 3 and (cases[n]["keys"] < 1 << 31).sum() > n_keys // 3
    k = cases["id_range"]["keys"]
    assert np.isin([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], k).all() and (k >= 1 << 31).sum() == 1002
    first = cases["id_range"]["steps"][0][1]
    assert first[0] == 0x80000000 and first[1] == 0  # local id 0 and key 0 are different things
    inter = cases["interleaved_clusters"]
    h = homes["interleaved_clusters"]
    assert (h[0::2] == 777).all() and (h[1::2] == 778).all() and len(inter["steps"]) == 2
    assert (inter["steps"][0][1][:500] == inter["keys"]).all()  # both clusters arrive in one fill, alternating
    # `grouped`: the occurrences of a key are adjacent
    g = cases["one_home_slot"]["steps"][2][1]
    assert (np.diff(np.flatnonzero(np.diff(g.astype(np.int64)) != 0)) >= 1).all()
    assert len(np.flatnonzero(np.diff(g.astype(np.int64)) != 0)) + 1 == len(np.unique(g))


def test_generation_case_has_its_properties():
    c = R.generation_case()
    keys, cap = c["keys"], c["capacity"]
    assert len(np.unique(keys)) == 400 and len(np.unique(R.global_slot(keys, cap))) == 1 and len(c["gens"]) == 21
    subsets = []
    for uniq, items in c["gens"]:
        final = _replay_case([("unique", uniq), ("dup", items)])
        assert np.isin(final, keys).all() and len(final) < 400 and len(items) <= 4000
        subsets.append(tuple(final))
    assert len(set(subsets)) == 21 and len({frozenset(s) for s in subsets}) == 21  # other subsets, other orders


def test_reference_agrees_with_the_oracle_table(oracle):
    rng = np.random.default_rng(5)
    num_node = 5000
    oht = oracle.HashTable(num_node, 5000)
    seeds = rng.permutation(num_node)[:300].astype(np.uint32)
    assert oht.fill_unique(seeds) == 0
    known = seeds
    for n in (1, 2500, 4000):
        items = np.minimum((num_node * rng.random(n) ** 2).astype(np.uint32), num_node - 1)
        uniq = oht.fill_duplicates(items)
        u, m = R.first_occurrence_dedup(known, items)
        np.testing.assert_array_equal(u, uniq)
        np.testing.assert_array_equal(m, oht.map_edges(items, items)[1])
        known = u


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("name", list(R.FLAT_CASES))
def test_sampler_cases_are_in_their_regimes(oracle, name, shape):
    case = R.sampler_case(name, shape)
    assert case["fanouts"][0] <= 600 and len(case["batches"]) == 2
    fills = R.sampler_regimes(oracle, case, R.SAMPLER_KINDS[shape])
    R.check_regimes(name, case, fills)
    assert max(fb["total"] for fb in fills) < 200000


@pytest.mark.parametrize("name", R.CROSS_CASES)
def test_cross_fill_cases_fall_back_where_they_claim(oracle, name):
    """khop1: the first fill's crowded bin falls back; in the last fill the same keys, now known, fall back again or are
    LDS-resident -- both read off the oracle's output, per fill"""
    case = R.cross_fill_case(name)
    fills = R.sampler_regimes(oracle, case, "KHOP1")
    R.check_regimes(name, case, fills)
    for fb in fills:
        assert fb["first"]["total"] == 13200 and fb["first"]["distinct"][R.BIN_A] > R.PARAMS["lds_limit"]
        assert fb["total"] < (1 << 16 if name == "falls_back_twice" else 1 << 17)


@pytest.mark.parametrize("kind", ["KHOP0", "KHOP2"])
def test_global_collision_case(oracle, kind):
    case = R.global_collision_case()
    cap = case["capacity"]
    assert cap == R.table_capacity(case["max_nodes"]) and cap >= 2 * case["max_nodes"]
    homes = R.global_slot(case["pool"], cap)
    assert set(homes) == set(np.arange(cap - 6, cap + 6) % cap)
    wants = []
    R.sampler_regimes(oracle, {**case, "expect": {}}, kind, want_out=wants)
    for want in wants:
        mids = want["input_nodes"][case["max_batch"]:want["graphs"][1]["num_src"]]
        assert len(mids) == 48 and np.isin(mids, case["pool"]).all()
        length, wraps = R.global_collision_stats(case, want)
        assert wraps and length >= 300, (length, wraps)
        assert len(np.unique(R.part_bin(mids, 5))) <= 2  # the last fill is lopsided for the partition as well
