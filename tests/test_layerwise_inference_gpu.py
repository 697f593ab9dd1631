"""examples/inference.py's layerwise_inference on the GPU (aggregation by fgnn_csr_aggregate) on an R-MAT graph of about
4000 nodes with one planted hub row longer than the kernel's split length: against the models' own forward on "full"
blocks on the GPU and against the float64 op-by-op pass on the CPU, both within rtol 1e-4 / atol 1e-4 -- the tolerance
the fused layers state against their op-by-op twins (tests/test_fused_gnn_gpu.py); fp16 features; chunk sizes; and
Accuracy(exact=True), which must not depend on a seed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from test_layerwise_inference_host import full_blocks  # noqa: E402

pytestmark = pytest.mark.gpu
N, E, HIDDEN, CLASSES, HUB_NODE = 4000, 60000, 64, 7, 1234
DIMS = (100, 128)


@pytest.fixture(scope="module")
def graph():
    """R-MAT CSR with row HUB_NODE replaced by 1.5 split lengths of distinct neighbours"""
    from fgnn_hip import nn, rmat
    assert torch.cuda.is_available()
    indptr, indices, _ = rmat.rmat_csr(N, E, seed=7)
    indptr, indices = indptr.numpy().view(np.uint32).astype(np.int64), indices.numpy().view(np.uint32)
    hub_len = nn.csr_split_length() * 3 // 2
    assert hub_len < N
    hub = np.random.default_rng(2).permutation(N)[:hub_len].astype(np.uint32)
    a, b = indptr[HUB_NODE], indptr[HUB_NODE + 1]
    indices = np.concatenate([indices[:a], hub, indices[b:]])
    indptr[HUB_NODE + 1:] += hub_len - (b - a)
    assert np.diff(indptr).max() == hub_len
    feats = {d: torch.from_numpy(np.random.default_rng(d).standard_normal((N, d)).astype(np.float32)) for d in DIMS}
    return indptr.astype(np.uint32), indices, feats


def _model(name, fused, dim, seed=1):
    from models import MODELS
    torch.manual_seed(seed)
    return MODELS[name](dim, HIDDEN, CLASSES, 2, 0.5, fused=fused)


_REF64 = {}


def _ref64(graph, name, fused, dim):
    """the float64 op-by-op pass on the CPU over the same parameters, once per model"""
    from inference import layerwise_inference
    key = (name, fused, dim)
    if key not in _REF64:
        indptr, indices, feats = graph
        _REF64[key] = layerwise_inference(_model(name, fused, dim).double(), indptr, indices, feats[dim].double())
    return _REF64[key]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
@pytest.mark.parametrize("name", ["graphsage", "gcn"])
def test_equals_the_full_block_forward_and_the_float64_pass(graph, name, fused, dim):
    from inference import layerwise_inference
    indptr, indices, feats = graph
    model = _model(name, fused, dim).cuda()
    model.train()
    got = layerwise_inference(model, indptr, indices, feats[dim])
    assert model.training and got.is_cuda and got.shape == (N, CLASSES) and got.dtype == torch.float32
    model.eval()
    with torch.no_grad():
        want = model(full_blocks(indptr, indices, 2, device="cuda"), feats[dim].cuda())
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    ref = _ref64(graph, name, fused, dim)
    torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", ["graphsage", "gcn"])
def test_half_features_are_read_as_they_are(graph, name):
    from inference import layerwise_inference
    indptr, indices, feats = graph
    dim = 128
    model = _model(name, True, dim).cuda()
    half = feats[dim].half()
    got = layerwise_inference(model, indptr, indices, half.cuda())
    want = layerwise_inference(model, indptr, indices, half.float().cuda())
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    # the first layer's sums see the same values in the same order: only the self rows' copy differs in kind, not value
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["graphsage", "gcn"])
def test_chunk_size_does_not_matter(graph, name):
    """batch_rows 257 and 4096 within rtol 1e-5 (atol 1e-5): the aggregation is bitwise the same, the GEMMs may pick
    different kernels"""
    from inference import layerwise_inference
    indptr, indices, feats = graph
    model = _model(name, True, 100).cuda()
    a = layerwise_inference(model, indptr, indices, feats[100], batch_rows=257)
    b = layerwise_inference(model, indptr, indices, feats[100], batch_rows=4096)
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


def test_exact_accuracy_equals_the_float64_predictions_and_ignores_the_seed(graph):
    import train_accuracy
    indptr, indices, feats = graph
    dim = 100
    model = _model("graphsage", True, dim, seed=5).cuda()
    from inference import layerwise_inference
    ref = layerwise_inference(_model("graphsage", True, dim, seed=5).double(), indptr, indices, feats[dim].double())
    top2 = ref.topk(2, dim=1).values
    clear = ((top2[:, 0] - top2[:, 1]) > 1e-3).numpy()
    rng = np.random.default_rng(3)
    label = ref.argmax(1).numpy().copy()
    flip = rng.random(N) < 0.4
    label[flip] = rng.integers(0, CLASSES, size=int(flip.sum()))
    test_set = np.flatnonzero(clear)[rng.permutation(int(clear.sum()))[:1500]].astype(np.uint32)
    assert len(test_set) == 1500
    want = float((ref.argmax(1).numpy()[test_set] == label[test_set]).mean())
    assert 0.5 < want < 0.9
    accs = []
    for seed in (1, 0xBEEF):
        acc = train_accuracy.Accuracy((indptr, indices), test_set[:100], test_set, feats[dim].numpy(),
                                      label.astype(np.uint64), [10, 5], 512, "cuda:0", seed=seed, exact=True)
        assert not hasattr(acc, "sampler")
        accs.append(acc.test_acc(model, "cuda:0"))
    assert accs[0] == accs[1] == want
