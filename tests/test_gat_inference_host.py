"""CPU-only: examples/inference.py's gat_layerwise_inference on the 300-node graph of
tests/test_layerwise_inference_host.py equals the GAT model's own forward on "full" blocks (one per layer, every node a
destination with its whole CSR row) for fused and op-by-op layer classes, with and without residual; fp16 features,
float64 models, the node without a neighbour; full_graph_inference dispatches by the model's class; Accuracy(exact=True)
takes a GAT model.  Tolerance: that file's, rtol 1e-5 with atol 1e-5."""
import numpy as np
import pytest
import torch

from test_layerwise_inference_host import CLASSES, D, HIDDEN, N, full_blocks, small_graph


@pytest.fixture(scope="module")
def graph():
    indptr, indices = small_graph()
    feat = torch.from_numpy(np.random.default_rng(6).standard_normal((N, D)).astype(np.float32))
    return indptr, indices, feat


def _gat(layers, fused, residual, seed=1, **kw):
    from models import GAT
    torch.manual_seed(seed)
    model = GAT(D, HIDDEN, CLASSES, layers, 0.5, fused=fused, heads=4, out_heads=2, residual=residual, **kw)
    with torch.no_grad():  # biases start at zero: give them values, so that a forgotten bias shows
        for layer in model.layers:
            layer.bias.normal_()
    return model


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
@pytest.mark.parametrize("layers", [2, 3])
def test_equals_the_models_forward_on_full_blocks(graph, layers, fused, residual):
    from inference import gat_layerwise_inference
    indptr, indices, feat = graph
    model = _gat(layers, fused, residual)
    model.eval()
    with torch.no_grad():
        want = model(full_blocks(indptr, indices, layers), feat)
    for training in (True, False):
        model.train(training)
        for batch_rows in (65536, 64, 7):
            got = gat_layerwise_inference(model, indptr, indices, feat, batch_rows=batch_rows)
            assert model.training is training
            assert got.shape == (N, CLASSES) and got.dtype == torch.float32 and not got.requires_grad
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


def test_takes_tensors_half_features_and_float64_models(graph):
    from inference import gat_layerwise_inference
    indptr, indices, feat = graph
    model = _gat(2, True, True, seed=2)
    t_indptr, t_indices = (torch.from_numpy(a.view(np.int32)) for a in (indptr, indices))
    want = gat_layerwise_inference(model, indptr, indices, feat)
    assert torch.equal(gat_layerwise_inference(model, t_indptr, t_indices, feat), want)
    # fp16 features are the same as their upcast
    half = gat_layerwise_inference(model, indptr, indices, feat.half())
    assert torch.equal(half, gat_layerwise_inference(model, indptr, indices, feat.half().float()))
    # a float64 model computes in float64
    got64 = gat_layerwise_inference(model.double(), indptr, indices, feat)
    assert got64.dtype == torch.float64
    torch.testing.assert_close(got64.float(), want, rtol=1e-5, atol=1e-5)


def test_a_node_without_a_neighbour_gets_residual_and_bias_only(graph):
    """node 7 has no neighbour: its logits are the last layer's bias averaged over the heads -- plus, with a residual,
    res_fc of its hidden row (layer 0's output, here from the model's own layer on a full block)"""
    from inference import gat_layerwise_inference
    indptr, indices, feat = graph
    assert indptr[8] == indptr[7]
    for residual in (False, True):
        model = _gat(2, False, residual, seed=3)
        model.eval()
        last = model.layers[1]
        assert (last.res_fc is not None) is residual
        with torch.no_grad():
            hidden = model.layers[0](full_blocks(indptr, indices, 1)[0], feat).flatten(1)
            want = last.bias.view(last.num_heads, last.out_feats)
            if residual:
                want = want + last.res_fc(hidden[7:8]).view(last.num_heads, last.out_feats)
            assert want.abs().min() > 0
        got = gat_layerwise_inference(model, indptr, indices, feat)
        torch.testing.assert_close(got[7], want.mean(0), rtol=1e-5, atol=1e-5)


def test_full_graph_inference_dispatches_by_the_models_class(graph):
    from inference import full_graph_inference, gat_layerwise_inference, layerwise_inference
    from models import MODELS
    indptr, indices, feat = graph
    torch.manual_seed(4)
    sage = MODELS["graphsage"](D, HIDDEN, CLASSES, 2, 0.5)
    assert torch.equal(full_graph_inference(sage, indptr, indices, feat, batch_rows=64),
                       layerwise_inference(sage, indptr, indices, feat, batch_rows=64))
    gat = _gat(2, True, False, seed=4)
    assert torch.equal(full_graph_inference(gat, indptr, indices, feat, batch_rows=64),
                       gat_layerwise_inference(gat, indptr, indices, feat, batch_rows=64))
    with pytest.raises(NotImplementedError) as e:
        layerwise_inference(gat, indptr, indices, feat)
    assert "edge-softmax" in str(e.value) and "gat_layerwise_inference" in str(e.value)
    for fn in (full_graph_inference, gat_layerwise_inference):
        with pytest.raises(NotImplementedError):
            fn(MODELS["pinsage"](D, HIDDEN, CLASSES, 2, 0.5), indptr, indices, feat)


def test_exact_accuracy_takes_a_gat_model(graph):
    """Accuracy(exact=True) on CPU tensors: the accuracy of the argmax of gat_layerwise_inference on the set's nodes,
    whatever the seed"""
    import train_accuracy
    from inference import gat_layerwise_inference
    indptr, indices, feat = graph
    model = _gat(2, True, True, seed=5)
    rng = np.random.default_rng(8)
    label = rng.integers(0, CLASSES, size=N).astype(np.uint64)
    valid, test = rng.permutation(N)[:50].astype(np.uint32), rng.permutation(N)[:80].astype(np.uint32)
    pred = gat_layerwise_inference(model, indptr, indices, feat).argmax(1).numpy()
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
