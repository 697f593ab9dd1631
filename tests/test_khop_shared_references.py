"""The sampling LAW of the shared-key sampler, on its numpy restatement tests/khop_shared_refs.py (the kernel is held to
it bit for bit by tests/test_khop_shared_gpu.py and tests/test_khop_shared_driver_gpu.py).  DESIGN.md 4.13 claims: each
seed's sample is a uniform fanout-subset (khop0's marginal distribution); seeds with overlapping rows prefer the same
neighbours; the words are fresh per (batch, layer) and belong to the NODE, not to the seed.  Modelled on
tests/test_oracle_distributions.py: fixed seeds, chi-square quantile at p = 1e-9, the same scaling.  CPU only."""
import numpy as np
from scipy.stats import chi2

import khop_shared_refs as refs
from ht_refs import first_occurrence_dedup
from train_refs import philox_blocks

SEED = 0x5A4D47
DEG = 12          # entries of every sampled row
NUM_SEEDS = 1500  # seed i = node DEG * NUM_SEEDS + i has the row [DEG * i, DEG * i + DEG): disjoint between seeds
FANOUT = 5


def _disjoint_rows():
    num_node = DEG * NUM_SEEDS + NUM_SEEDS
    indptr = np.concatenate([np.zeros(DEG * NUM_SEEDS, np.int64), np.arange(NUM_SEEDS + 1) * DEG]).astype(np.uint32)
    indices = np.arange(DEG * NUM_SEEDS, dtype=np.uint32)
    return indptr, indices, np.arange(DEG * NUM_SEEDS, num_node, dtype=np.uint32)


def _inclusion_statistic():
    """chi-square statistic of the inclusion counts per row position over 4 batch keys x both layers' tags, and its limit"""
    indptr, indices, seeds = _disjoint_rows()
    counts, calls = np.zeros(DEG), 0
    for batch_key in (100, 101, 2**40 + 5, 103):
        for layer in (0, 1):
            src, dst = refs.sample(indptr, indices, seeds, FANOUT, SEED, batch_key, layer)
            assert len(dst) == NUM_SEEDS * FANOUT and (dst // DEG + DEG * NUM_SEEDS == src).all()
            per_seed = dst.reshape(NUM_SEEDS, FANOUT)
            assert (per_seed[:, 1:] > per_seed[:, :-1]).all()  # CSR order, no repeats
            counts += np.bincount(dst % DEG, minlength=DEG)
            calls += 1
    p = FANOUT / DEG
    expected = np.full(DEG, calls * NUM_SEEDS * p)
    # inclusion counts of independent simple random samples: covariance B p (1-p) n/(n-1) (I - J/n)
    stat = float(((counts - expected) ** 2 / (expected * (1 - p) * DEG / (DEG - 1))).sum())
    return stat, float(chi2.isf(1e-9, DEG - 1)), counts


def test_inclusion_is_uniform():
    stat, limit, counts = _inclusion_statistic()
    assert stat < limit, (stat, limit, counts)


def test_a_wrong_word_of_the_block_fails_the_uniformity_check(monkeypatch):
    """the check has teeth: with word 0 of the block for all four ids of a block, the ids 4b .. 4b + 3 of a row tie and
    the position decides -- the first position of each group of four is kept far too often"""
    def word_zero(num_node, seed, batch_key, layer):
        blocks = philox_blocks(seed, batch_key, refs.KHOP_SHARED << 8 | layer & 0xFF, (num_node + 3) // 4)
        return np.repeat(blocks[:, 0], 4)[:num_node]
    monkeypatch.setattr(refs, "node_words", word_zero)
    stat, limit, counts = _inclusion_statistic()
    assert stat > 10 * limit, (stat, limit, counts)


def _graph(num_node, rows):
    lens = np.zeros(num_node, dtype=np.int64)
    lens[:len(rows)] = [len(r) for r in rows]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), np.concatenate(rows).astype(np.uint32)


def _picks(indptr, indices, seeds, fanout, batch_key, layer, **kw):
    """{seed: tuple of its destinations in output order}"""
    src, dst = refs.sample(indptr, indices, seeds, fanout, SEED, batch_key, layer, **kw)
    return {int(s): tuple(dst[src == s].tolist()) for s in np.unique(src)}


def test_nesting_and_permutations_are_exact():
    """rows with distinct ids, longer than the fanout.  A a sub-multiset of B: what B keeps of A's ids, A keeps too (an
    id among the k smallest words of B is among the k smallest of any subset that holds it).  Rows that are permutations of
    each other keep the same set."""
    rng = np.random.default_rng(21)
    num_node, fanout, pairs = 6000, 7, 300
    rows = []
    for _ in range(pairs):
        b = rng.permutation(num_node)[:30]
        a = rng.permutation(b)[:int(rng.integers(fanout + 1, 25))]  # a subset of B in an order of its own
        rows += [b, a, rng.permutation(b)]
    indptr, indices = _graph(num_node, rows)
    seeds = np.arange(len(rows), dtype=np.uint32)
    shared = 0
    for batch_key, layer in ((7, 0), (7, 1), (8, 0)):
        words = refs.node_words(num_node, SEED, batch_key, layer)
        assert len(np.unique(words)) == num_node  # no two ids tie: the statements below are about words alone
        picks = _picks(indptr, indices, seeds, fanout, batch_key, layer)
        for p in range(pairs):
            got_b, got_a, got_perm = (set(picks[3 * p + i]) for i in range(3))
            assert len(got_b) == len(got_a) == fanout
            assert got_b & set(rows[3 * p + 1].tolist()) <= got_a, (batch_key, layer, p)
            assert got_perm == got_b, (batch_key, layer, p)
            shared += len(got_a & got_b)
    # the point of the sampler: A keeps every id that B keeps of it, about 7 * |A| / 30 of them, where two independent
    # 7-subsets of A and B would share 49 / 30
    assert shared > 2 * pairs * 3, shared


def test_words_are_fresh_per_batch_and_layer_and_belong_to_the_node():
    num_node = 20000
    words = {(k, l): refs.node_words(num_node, SEED, k, l) for k in (1, 2, 2**33 + 1) for l in (0, 1)}
    keys = list(words)
    for i, a in enumerate(keys):
        assert len(np.unique(words[a])) > 0.999 * num_node, a  # a word of its own for every node of a block, too
        for b in keys[i + 1:]:
            assert (words[a] == words[b]).mean() < 1e-3, (a, b)
    # a seed's picks depend on (batch key, layer) and its row only: not on the seed list, its order or src_local
    rng = np.random.default_rng(22)
    rows = [rng.integers(0, num_node, int(n)) for n in rng.integers(0, 60, 400)]
    indptr, indices = _graph(num_node, rows)
    seeds = np.arange(400, dtype=np.uint32)
    full = _picks(indptr, indices, seeds, 6, 5, 1)
    part_seeds = rng.permutation(400)[:150].astype(np.uint32)
    part = _picks(indptr, indices, part_seeds, 6, 5, 1)
    assert part == {s: full[s] for s in part}
    src_g, dst_g = refs.sample(indptr, indices, part_seeds, 6, SEED, 5, 1)
    src_l, dst_l = refs.sample(indptr, indices, part_seeds, 6, SEED, 5, 1, src_local=True)
    np.testing.assert_array_equal(dst_g, dst_l)
    np.testing.assert_array_equal(part_seeds[src_l], src_g)
    assert full != _picks(indptr, indices, seeds, 6, 6, 1) and full != _picks(indptr, indices, seeds, 6, 5, 0)


def test_ties_are_decided_by_position():
    """equal words (a row that repeats an id): the earlier position wins"""
    words = refs.node_words(1000, SEED, 3, 0)
    assert len(np.unique(words)) == 1000
    for k in (1, 5, 25, 64):
        np.testing.assert_array_equal(refs.keep(np.full(2 * k + 2, 777), words, k), np.arange(k))
    # among other ids: of the id that straddles the threshold, its first occurrences are kept
    rng = np.random.default_rng(23)
    for trial in range(200):
        row = rng.choice(rng.permutation(1000)[:6], 40)
        k = int(rng.integers(1, 39))
        kept = refs.keep(row, words, k)
        assert len(kept) == k and (np.diff(kept) > 0).all()
        order = np.argsort(words[np.unique(row)], kind="stable")
        left = k
        for t in np.unique(row)[order]:  # ids by ascending word (distinct ids have distinct words here)
            at = np.flatnonzero(row == t)
            take = min(left, len(at))
            assert np.isin(at[:take], kept).all() and not np.isin(at[take:], kept).any(), (trial, t)
            left -= take


def test_reference_batch_numbers_nodes_like_the_dedup_table():
    """reference_batch on a small graph, against a walk written out by hand: frontier = all nodes so far, new
    destinations numbered by first occurrence"""
    rng = np.random.default_rng(24)
    num_node = 300
    rows = [rng.integers(0, num_node, int(n)) for n in rng.integers(0, 20, num_node)]
    indptr, indices = _graph(num_node, rows)
    seeds, fanouts = rng.permutation(num_node)[:17].astype(np.uint32), [4, 3]
    want = refs.reference_batch(indptr, indices, seeds, fanouts, SEED, 9)
    nodes = want["input_nodes"]
    assert (nodes[:17] == seeds).all() and len(np.unique(nodes)) == len(nodes)
    g1, g0 = want["graphs"][1], want["graphs"][0]
    assert (g1["num_dst"], g0["num_dst"], g0["num_src"]) == (17, g1["num_src"], len(nodes))
    for l, g in enumerate(want["graphs"]):
        src, dst = refs.sample(indptr, indices, nodes[:g["num_dst"]], fanouts[l], SEED, 9, l)
        np.testing.assert_array_equal(nodes[g["col"]], src)
        np.testing.assert_array_equal(nodes[g["row"]], dst)
        assert g["num_edge"] == len(dst) and (g["row"] < g["num_src"]).all()
        new = g["row"][g["row"] >= g["num_dst"]]
        first = new[np.sort(np.unique(new, return_index=True)[1])]
        np.testing.assert_array_equal(first, np.arange(g["num_dst"], g["num_src"]))  # numbered as they first appear
    refs.check_batch(indptr, indices, nodes, [(g["row"], g["col"], g["num_src"], g["num_dst"]) for g in want["graphs"]],
                     fanouts, seeds, SEED, 9)
    assert first_occurrence_dedup(seeds, [])[0].tolist() == seeds.tolist()
