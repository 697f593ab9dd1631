"""CPU-only: examples/inference.py's layerwise_inference on a 300-node graph equals the model's own forward on "full"
blocks -- one per layer, every node a destination with its whole CSR row: row = indices, col = repeat(arange(N), deg),
num_src = num_dst = N -- for SAGE and GCN with fused and op-by-op layer classes; PinSAGE and GAT are refused with a
reason; the model's training flag comes back.  Tolerance: rtol 1e-5 (with atol 1e-5 on outputs of order 1, the way this
suite states a relative tolerance with torch.testing.assert_close)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

N, D, HIDDEN, CLASSES = 300, 24, 16, 5


def full_blocks(indptr, indices, layers, device="cpu", dtype=torch.int32):
    from samgraph.torch.adapter import CooBlock
    n = len(indptr) - 1
    row = torch.from_numpy(indices.astype(np.int64)).to(dtype).to(device)
    col = torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(indptr.astype(np.int64)))).to(dtype).to(device)
    return [CooBlock(row, col, n, n) for _ in range(layers)]


def small_graph(n=N, seed=4):
    """rows of 0 .. 12 neighbours, one row of 150; some nodes are nobody's neighbour (out-degree 0)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 13, size=n)
    k[7], k[8] = 0, 150
    indptr = np.concatenate([[0], np.cumsum(k)]).astype(np.uint32)
    indices = rng.integers(0, n - 20, size=int(k.sum())).astype(np.uint32)
    return indptr, indices


@pytest.fixture(scope="module")
def graph():
    indptr, indices = small_graph()
    feat = torch.from_numpy(np.random.default_rng(6).standard_normal((N, D)).astype(np.float32))
    return indptr, indices, feat


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
@pytest.mark.parametrize("name", ["graphsage", "gcn"])
@pytest.mark.parametrize("layers", [2, 3])
def test_equals_the_models_forward_on_full_blocks(graph, name, fused, layers):
    from inference import layerwise_inference
    from models import MODELS
    indptr, indices, feat = graph
    torch.manual_seed(1)
    model = MODELS[name](D, HIDDEN, CLASSES, layers, 0.5, fused=fused)
    model.eval()
    with torch.no_grad():
        want = model(full_blocks(indptr, indices, layers), feat)
    for training in (True, False):
        model.train(training)
        for batch_rows in (65536, 64, 7):
            got = layerwise_inference(model, indptr, indices, feat, batch_rows=batch_rows)
            assert model.training is training
            assert got.shape == (N, CLASSES) and got.dtype == torch.float32 and not got.requires_grad
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


def test_takes_tensors_half_features_and_float64_models(graph):
    from inference import layerwise_inference
    from models import MODELS
    indptr, indices, feat = graph
    torch.manual_seed(2)
    model = MODELS["graphsage"](D, HIDDEN, CLASSES, 2, 0.0)
    t_indptr, t_indices = (torch.from_numpy(a.view(np.int32)) for a in (indptr, indices))
    want = layerwise_inference(model, indptr, indices, feat)
    assert torch.equal(layerwise_inference(model, t_indptr, t_indices, feat), want)
    # fp16 features are the same as their upcast
    half = layerwise_inference(model, indptr, indices, feat.half())
    assert torch.equal(half, layerwise_inference(model, indptr, indices, feat.half().float()))
    # a float64 model computes in float64
    got64 = layerwise_inference(model.double(), indptr, indices, feat)
    assert got64.dtype == torch.float64
    torch.testing.assert_close(got64.float(), want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", ["pinsage", "gat"])
def test_models_without_a_csr_neighbourhood_are_refused_with_a_reason(graph, name):
    from inference import layerwise_inference
    from models import MODELS
    indptr, indices, feat = graph
    model = MODELS[name](D, HIDDEN, CLASSES, 2, 0.5)
    model.train()
    with pytest.raises(NotImplementedError) as e:
        layerwise_inference(model, indptr, indices, feat)
    assert ("random walks" if name == "pinsage" else "edge-softmax") in str(e.value)
    assert model.training


def test_exact_accuracy_needs_no_sampler_and_no_gpu(graph):
    """Accuracy(exact=True) on CPU tensors: the accuracy of the full-graph predictions on the set's nodes, whatever
    the seed"""
    import train_accuracy
    from inference import layerwise_inference
    from models import MODELS
    indptr, indices, feat = graph
    torch.manual_seed(3)
    model = MODELS["gcn"](D, HIDDEN, CLASSES, 2, 0.5)
    rng = np.random.default_rng(8)
    label = rng.integers(0, CLASSES, size=N).astype(np.uint64)
    valid, test = rng.permutation(N)[:50].astype(np.uint32), rng.permutation(N)[:80].astype(np.uint32)
    pred = layerwise_inference(model, indptr, indices, feat).argmax(1).numpy()
    accs = []
    for seed in (1, 2):
        acc = train_accuracy.Accuracy((indptr, indices), valid, test, feat.numpy(), label, [5, 5], 32, "cpu", seed=seed,
                                      exact=True)
        model.train()
        accs.append((acc.valid_acc(model, "cpu"), acc.test_acc(model, "cpu")))
        assert model.training
    assert accs[0] == accs[1]
    assert accs[0] == ((pred[valid] == label[valid].astype(np.int64)).mean(),
                       (pred[test] == label[test].astype(np.int64)).mean())
