"""CPU-only: the float64 reference and the measured bound that tests/test_csr_gat_gpu.py holds the CSR GAT kernel to
(tests/csr_gat_refs.py) are sound -- the reference agrees with gat_refs.gat_ref on the rows' COO expansion, the
piecewise combination the kernel is defined by equals the softmax in one run, and no case's bound is trivial."""
import numpy as np
import pytest

import csr_gat_refs as G
import csr_refs
import gat_refs

SPLIT = 1024  # the kernel's piece length today; nothing here needs the two to match
CASES = [(H, F, "normal") for H, F in gat_refs.HEADS_FEATS] + [(8, 32, "overflow"), (3, 7, "overflow")]


@pytest.mark.parametrize("kind", ["normal", "overflow"])
def test_reference_equals_gat_ref_on_the_coo_expansion(kind):
    """a few special rows (empty, 1, 3, 33, 65, split + 1 edges) with er gathered per destination"""
    H, F = 3, 7
    indptr, indices = G.graph(SPLIT)
    lengths = csr_refs.special_lengths(SPLIT)
    rows = csr_refs.SPECIAL_AT + np.array([lengths.index(k) for k in (0, 1, 3, 33, 65, SPLIT + 1)])
    el, er = G.scores(H, kind)
    feat = G.feat_view(H, F)
    got = G.csr_gat_ref(indptr, indices, feat, el, er, rows)
    row, col, srcs = G.coo_of_rows(indptr, indices, rows)
    want = gat_refs.gat_ref(row, col, feat[srcs], el[srcs], er[rows], len(rows))["out"]
    assert (got[0] == 0).all() and np.abs(got[1:]).min() > 0
    one = int(indices[indptr[rows[1]]])
    np.testing.assert_array_equal(got[1], feat[one].astype(np.float64))  # one edge: its weight is 1
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("kind", ["normal", "overflow"])
@pytest.mark.parametrize("k", [1, SPLIT, SPLIT + 1, 3 * SPLIT + 5])
def test_piecewise_combination_equals_the_softmax_in_one_run(k, kind):
    rs = np.random.default_rng(k)
    H, F = 4, 5
    s = rs.uniform(-100, 100, (k, H)) if kind == "overflow" else rs.standard_normal((k, H))
    feat = rs.standard_normal((k, H, F))
    p = np.exp(s - s.max(axis=0))
    want = ((p / p.sum(axis=0))[:, :, None] * feat).sum(axis=0)
    got = G.piecewise_combination(s, feat, SPLIT)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%s" % c)
def test_the_bound_is_not_trivial(case):
    """the torch fp32 formulation deviates from the reference on the rows of more than one edge (so 4 x deviation is a
    bound a kernel can miss), stays finite, and the bound is far below the data's scale"""
    H, F, kind = case
    ref, bound, dev, t32 = G.expectation(H, F, kind, SPLIT)
    k = np.diff(G.graph(SPLIT)[0].astype(np.int64))[csr_refs.special_rows(SPLIT)]
    assert ref.shape == (len(k), H, F) and np.isfinite(ref).all() and np.isfinite(t32).all()
    long_dev = np.abs(t32.astype(np.float64) - ref)[k > 1].max()
    print("%dx%d %s: torch fp32 deviation %.3g (rows of more than one edge: %.3g)" % (H, F, kind, dev, long_dev))
    assert long_dev > 0 and dev >= long_dev
    assert (ref[k == 0] == 0).all() and (k == 0).sum() >= 5
    assert 0 < bound.max() < 1e-3 * np.abs(ref).max()
