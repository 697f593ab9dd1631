"""Plain numpy restatement of the shared-key sampler (csrc/sample_khop_shared.hip), compared for equality."""
import numpy as np

from ht_refs import first_occurrence_dedup
from train_refs import philox_blocks

KHOP_SHARED = 8


def node_words(num_node, seed, batch_key, layer):
    """uint32[num_node]: node t's word = word t & 3 of the Philox block (item t >> 2, block 0) of (type 8, layer)"""
    return philox_blocks(seed, batch_key, KHOP_SHARED << 8 | layer & 0xFF, (num_node + 3) // 4).reshape(-1)[:num_node]


def _kept(seg, start, ids, words, fanout):
    """mask over rows laid end to end (entry e: row seg[e], node id ids[e]; row r is entries start[r] .. start[r + 1]):
    an entry is kept iff its key (word of the neighbour << 32 | position in the row) is no larger than the row's
    `fanout`-th smallest key -- than its largest, if the row has no more than `fanout` entries"""
    e = np.arange(len(ids), dtype=np.int64)
    key = (words[ids].astype(np.uint64) << np.uint64(32)) | (e - start[seg]).astype(np.uint64)
    ascending = key[np.lexsort((key, seg))]  # seg is ascending: every row stays where it is, its keys sorted
    kth = start[:-1] + np.minimum(np.diff(start), fanout) - 1
    return key <= ascending[np.clip(kth, 0, None)][seg] if len(ids) else np.zeros(0, dtype=bool)


def keep(row, words, fanout):
    """ascending positions of one row (node ids) that a seed keeps"""
    row = np.asarray(row, dtype=np.int64)
    return np.flatnonzero(_kept(np.zeros(len(row), np.int64), np.array([0, len(row)]), row, words, fanout))


def sample(indptr, indices, seeds, fanout, seed, batch_key, layer, src_local=False):
    """(out_src, out_dst) uint32: per seed the kept entries of its row (_kept), in CSR order"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.uint32)
    seeds = np.asarray(seeds, dtype=np.int64)
    words = node_words(len(indptr) - 1, seed, batch_key, layer)
    lens = indptr[seeds + 1] - indptr[seeds]
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seg = np.repeat(np.arange(len(seeds), dtype=np.int64), lens)
    ids = indices[indptr[seeds][seg] + np.arange(start[-1], dtype=np.int64) - start[seg]]
    mask = _kept(seg, start, ids, words, fanout)
    return (seg if src_local else seeds[seg])[mask].astype(np.uint32), ids[mask]


def reference_batch(indptr, indices, seeds, fanouts, seed, batch_key):
    """a batch of the driver, laid out like oracle.do_sample's result: dict(input_nodes, graphs[l] = dict(row, col,
    num_edge, num_src, num_dst)).  The layers are sampled in the driver's order (engine.hip: the last one first, from the
    seeds; layer 0 last); a layer's frontier is every node known so far, col the local id of an edge's seed, row that of
    its destination -- new destinations are numbered behind the frontier in order of first occurrence, the numbering of
    the dedup table (ht_refs.first_occurrence_dedup).  The seeds are distinct."""
    nodes = np.asarray(seeds, dtype=np.uint32)
    graphs = [None] * len(fanouts)
    for l in range(len(fanouts) - 1, -1, -1):
        num_dst = len(nodes)
        col, dst = sample(indptr, indices, nodes, fanouts[l], seed, batch_key, l, src_local=True)
        nodes, row = first_occurrence_dedup(nodes, dst)
        graphs[l] = dict(row=row, col=col, num_edge=len(row), num_src=len(nodes), num_dst=num_dst)
    return dict(input_nodes=nodes, graphs=graphs)


def check_batch(indptr, indices, input_nodes, graphs, fanouts, seeds, seed, batch_key, want=None):
    """a batch of the driver: graphs[l] = (row, col, num_src, num_dst) local ids.  input_nodes and every layer's row and
    col equal reference_batch's (`want`, where the caller has it already), array for array: the fills keep the samplers'
    edge order and number new nodes by first occurrence, for this sampler as for every other."""
    if want is None:
        want = reference_batch(indptr, indices, seeds, fanouts, seed, batch_key)
    np.testing.assert_array_equal(input_nodes, want["input_nodes"])
    assert len(graphs) == len(fanouts)
    for l, (row, col, num_src, num_dst) in enumerate(graphs):
        g = want["graphs"][l]
        assert (len(row), num_src, num_dst) == (g["num_edge"], g["num_src"], g["num_dst"]), l
        np.testing.assert_array_equal(row, g["row"], err_msg="row of layer %d" % l)
        np.testing.assert_array_equal(col, g["col"], err_msg="col of layer %d" % l)
    return want
