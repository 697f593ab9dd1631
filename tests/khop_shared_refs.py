"""Plain numpy restatement of the shared-key sampler (csrc/sample_khop_shared.hip), compared for equality."""
import numpy as np

from train_refs import philox_blocks

KHOP_SHARED = 8


def node_words(num_node, seed, batch_key, layer):
    """uint32[num_node]: node t's word = word t & 3 of the Philox block (item t >> 2, block 0) of (type 8, layer)"""
    return philox_blocks(seed, batch_key, KHOP_SHARED << 8 | layer & 0xFF, (num_node + 3) // 4).reshape(-1)[:num_node]


def sample(indptr, indices, seeds, fanout, seed, batch_key, layer, src_local=False):
    """(out_src, out_dst) uint32: per seed, the whole row if it has at most `fanout` entries, else the `fanout`
    positions with the smallest (word of the neighbour << 32 | position), in CSR order"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.uint32)
    words = node_words(len(indptr) - 1, seed, batch_key, layer).astype(np.uint64)
    src, dst = [], []
    for i, s in enumerate(np.asarray(seeds, dtype=np.int64)):
        row = indices[indptr[s]:indptr[s + 1]]
        pos = np.arange(len(row), dtype=np.uint64)
        if len(row) > fanout:
            key = (words[row] << np.uint64(32)) | pos
            pos = np.sort(np.argsort(key, kind="stable")[:fanout])
        dst.append(row[pos.astype(np.int64)])
        src.append(np.full(len(pos), i if src_local else s, dtype=np.uint32))
    cat = (lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint32))
    return cat(src), cat(dst)


def check_batch(indptr, indices, input_nodes, graphs, fanouts, seeds, seed, batch_key):
    """a batch of the driver: graphs[l] = (row, col, num_src, num_dst) local ids.  input_nodes starts with the seeds and is
    duplicate-free; every layer's edges, as global ids, are the reference sample of that layer's frontier."""
    assert (input_nodes[:len(seeds)] == seeds).all() and len(np.unique(input_nodes)) == len(input_nodes)
    for l, (row, col, num_src, num_dst) in enumerate(graphs):
        frontier = input_nodes[:num_dst]
        want_src, want_dst = sample(indptr, indices, frontier, fanouts[l], seed, batch_key, l)
        got = sorted(zip(input_nodes[col].tolist(), input_nodes[row].tolist()))
        assert got == sorted(zip(want_src.tolist(), want_dst.tolist())), l
        assert num_src <= len(input_nodes) and (row < num_src).all()
