"""CPU-only: the float64 reference of the CSR aggregation (tests/csr_refs.py) is what the formula says -- on 4-node cases
computed by hand, and against the block aggregation's reference (tests/train_refs.py) on the same edges expanded to
COO -- and the synthetic graph of the GPU test has the rows it promises."""
import numpy as np
import pytest
import torch

import csr_refs
import train_refs

# 4 nodes: row 0 = {1, 2}, row 1 = {}, row 2 = {0, 1, 3}, row 3 = {3}
INDPTR = np.array([0, 2, 2, 5, 6], dtype=np.uint32)
INDICES = np.array([1, 2, 0, 1, 3, 3], dtype=np.uint32)
H = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]], dtype=np.float32)


def test_plain_sum_by_hand():
    ref, S, k = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H)
    assert ref.dtype == np.float64
    assert ref.tolist() == [[6.0, 60.0], [0.0, 0.0], [11.0, 110.0], [8.0, 80.0]]
    assert S.tolist() == ref.tolist() and k.tolist() == [2, 0, 3, 1]


def test_nodes_list_range_and_weights_by_hand():
    w = np.array([0.5, -1.0, 2.0, 1.0, 0.25, 3.0], dtype=np.float32)  # per CSR position
    ref, S, k = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H, nodes=[2, 0, 2], w=w)
    assert ref.tolist() == [[6.0, 60.0], [-3.0, -30.0], [6.0, 60.0]]  # 2*1 + 1*2 + .25*8; .5*2 - 1*4
    assert S.tolist() == [[6.0, 60.0], [5.0, 50.0], [6.0, 60.0]] and k.tolist() == [3, 2, 3]
    ref, _, k = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H, first=1, count=2)
    assert ref.tolist() == [[0.0, 0.0], [11.0, 110.0]] and k.tolist() == [0, 3]


def test_degree_modes_by_hand():
    src_deg = np.array([4.0, 0.25, 16.0, 1.0], dtype=np.float32)  # 0.25 clamps to 1
    dst_deg = np.array([4.0, 9.0, 0.0, 16.0], dtype=np.float32)   # indexed by node id; 0 clamps to 1
    ref, _, _ = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H, src_deg=src_deg, src_mode=1)
    assert ref[:, 0].tolist() == [2.0 + 4.0 / 4, 0.0, 1.0 / 2 + 2.0 + 8.0, 8.0]
    ref, _, _ = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H, src_deg=src_deg, src_mode=2)
    assert ref[:, 0].tolist() == [2.0 + 4.0 / 16, 0.0, 1.0 / 4 + 2.0 + 8.0, 8.0]
    ref, _, _ = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H, dst_deg=dst_deg, dst_mode=1)
    assert ref[:, 0].tolist() == [6.0 / 2, 0.0, 11.0, 8.0 / 4]
    ref, _, _ = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H, nodes=[3, 0], dst_deg=dst_deg, dst_mode=2)
    assert ref[:, 0].tolist() == [8.0 / 16, 6.0 / 4]
    # no degree vector: the row's own length (the mean; an empty row keeps factor 1)
    ref, _, _ = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H, dst_mode=2)
    assert ref[:, 0].tolist() == [3.0, 0.0, 11.0 / 3, 8.0]
    ref, _, _ = csr_refs.csr_aggregate_ref(INDPTR, INDICES, H, dst_mode=1)
    np.testing.assert_allclose(ref[:, 0], [6.0 / 2 ** 0.5, 0.0, 11.0 / 3 ** 0.5, 8.0], rtol=1e-15, atol=0)


def test_half_input_is_upcast_exactly():
    h16 = np.array([[0.1, 1 / 3], [65504.0, 6e-8], [-2.5, 0.0], [1e-3, 3.0]], dtype=np.float16)
    ref, _, _ = csr_refs.csr_aggregate_ref(INDPTR, INDICES, h16)
    want, _, _ = csr_refs.csr_aggregate_ref(INDPTR, INDICES, h16.astype(np.float64))
    assert ref.dtype == np.float64 and (ref == want).all()
    assert ref[0, 0] == float(h16[1, 0]) + float(h16[2, 0])


@pytest.mark.parametrize("modes", [(0, 0), (1, 1), (2, 0), (0, 2), (2, 1)])
@pytest.mark.parametrize("weighted", [False, True])
def test_equals_the_block_aggregation_reference_on_the_same_edges(modes, weighted):
    rng = np.random.default_rng(5)
    n, dim = 200, 7
    k = rng.integers(0, 9, size=n)
    k[17], k[18] = 0, 300
    indptr = np.concatenate([[0], np.cumsum(k)]).astype(np.uint32)
    indices = rng.integers(0, n, size=int(k.sum())).astype(np.uint32)
    h = rng.standard_normal((n, dim)).astype(np.float32)
    w = rng.standard_normal(len(indices)).astype(np.float32) if weighted else None
    src_deg = rng.uniform(0, 30, size=n).astype(np.float32)
    dst_deg = rng.uniform(0, 30, size=n).astype(np.float32)
    nodes = rng.permutation(n)[:150]
    pos, dst, kk = csr_refs.expand(indptr, nodes)
    # COO of the call: row = neighbour, col = output row; the block reference indexes dst_deg by output row
    row, col = torch.from_numpy(indices[pos].astype(np.int64)), torch.from_numpy(dst)
    want, want_S, want_k = train_refs.aggregate_ref(row, col, None if w is None else torch.from_numpy(w[pos]),
                                                    torch.from_numpy(h), len(nodes), torch.from_numpy(src_deg), modes[0],
                                                    torch.from_numpy(dst_deg[nodes]), modes[1])
    ref, S, got_k = csr_refs.csr_aggregate_ref(indptr, indices, h, nodes=nodes, w=w, src_deg=src_deg, src_mode=modes[0],
                                               dst_deg=dst_deg, dst_mode=modes[1])
    assert (got_k == want_k.numpy()).all() and (got_k == kk).all()
    np.testing.assert_allclose(ref, want.numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(S, want_S.numpy(), rtol=1e-13, atol=0)
    assert (csr_refs.aggregate_bound(S, got_k) == train_refs.aggregate_bound(torch.from_numpy(S),
                                                                            torch.from_numpy(got_k)).numpy()).all()


def test_synthetic_graph_has_the_promised_rows():
    split = 1024
    indptr, indices = csr_refs.synthetic_csr(split)
    assert indptr.dtype == np.uint32 and indices.dtype == np.uint32 and len(indptr) == csr_refs.NUM_NODE + 1
    k = np.diff(indptr.astype(np.int64))
    sp = csr_refs.special_lengths(split)
    assert k[csr_refs.SPECIAL_AT:csr_refs.SPECIAL_AT + len(sp)].tolist() == sp
    for want in (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, split - 1, split, split + 1, 3 * split + 5, 100_000):
        assert want in sp
    hub = csr_refs.SPECIAL_AT + sp.index(csr_refs.HUB)
    assert k[hub - 1] == 0 and k[hub + 1] == 0  # empty rows on both sides of the hub
    assert int(indices.max()) == csr_refs.NUM_NODE - 1 and len(indices) == int(k.sum())
    assert len(np.unique(indices[indptr[hub] + 1:indptr[hub + 1]])) == csr_refs.HUB - 1  # distinct neighbours
    rows = csr_refs.special_rows(split)
    assert rows[0] == csr_refs.SPECIAL_AT - 1 and rows[-1] == csr_refs.SPECIAL_AT + len(sp)
