"""examples/inference.py's gatv2_layerwise_inference.  Host part on the 300-node graph of
tests/test_layerwise_inference_host.py (its tolerance, 1e-5); GPU part on the graph of tests/test_gat_inference_gpu.py
(4000-node R-MAT with a planted hub of 1.5 split lengths, 8 heads x 8; its tolerances, 1e-4)."""
import numpy as np
import pytest
import torch

from test_gat_inference_gpu import CLASSES as G_CLASSES, DIM, HEADS, HIDDEN as G_HIDDEN, N as G_N, graph  # noqa: F401
from test_layerwise_inference_host import CLASSES, D, HIDDEN, N, full_blocks, small_graph


def _gatv2(dims, fused, out_heads, residual, share_weights, heads, seed=1):
    from models import GATv2
    torch.manual_seed(seed)
    model = GATv2(*dims, 2, 0.5, fused=fused, heads=heads, out_heads=out_heads, residual=residual,
                  share_weights=share_weights)
    with torch.no_grad():  # biases start at zero: give them values, so that a forgotten bias shows
        for layer in model.layers:
            for fc in (layer.fc_src, layer.fc_dst):
                if fc is not None:
                    fc.bias.normal_()
    return model


@pytest.mark.parametrize("share_weights", [False, True], ids=["two_fc", "shared"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
def test_host_equals_the_models_forward_on_full_blocks(fused, share_weights):
    from inference import full_graph_inference, gatv2_layerwise_inference, layerwise_inference
    indptr, indices = small_graph()
    feat = torch.from_numpy(np.random.default_rng(6).standard_normal((N, D)).astype(np.float32))
    model = _gatv2((D, HIDDEN, CLASSES), fused, 2, True, share_weights, heads=4)
    model.eval()
    with torch.no_grad():
        want = model(full_blocks(indptr, indices, 2), feat)
    for training in (True, False):
        model.train(training)
        got = full_graph_inference(model, indptr, indices, feat, batch_rows=64)
        assert model.training is training
        assert got.shape == (N, CLASSES) and got.dtype == torch.float32 and not got.requires_grad
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
        assert torch.equal(got, gatv2_layerwise_inference(model, indptr, indices, feat, batch_rows=64))
    with pytest.raises(NotImplementedError):
        layerwise_inference(model, indptr, indices, feat)


@pytest.mark.gpu
@pytest.mark.parametrize("share_weights", [False, True], ids=["two_fc", "shared"])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("out_heads", [1, 2])
def test_gpu_equals_the_full_block_forward_and_the_float64_pass(graph, out_heads, residual, share_weights):  # noqa: F811
    from inference import gatv2_layerwise_inference
    indptr, indices, feat = graph
    dims = (DIM, G_HIDDEN, G_CLASSES)
    model = _gatv2(dims, True, out_heads, residual, share_weights, HEADS).cuda()
    model.train()
    got = gatv2_layerwise_inference(model, indptr, indices, feat)
    assert model.training and got.is_cuda and got.shape == (G_N, G_CLASSES) and got.dtype == torch.float32
    model.eval()
    with torch.no_grad():
        want = model(full_blocks(indptr, indices, 2, device="cuda"), feat.cuda())
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    ref = gatv2_layerwise_inference(_gatv2(dims, True, out_heads, residual, share_weights, HEADS).double(), indptr,
                                    indices, feat.double())
    assert ref.dtype == torch.float64 and not ref.is_cuda
    torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_gpu_chunk_size_and_exact_accuracy(graph):  # noqa: F811
    """batch_rows 257 against 4096 (the GEMMs may pick different kernels); Accuracy(exact=True) whatever the seed"""
    import train_accuracy
    from inference import full_graph_inference
    indptr, indices, feat = graph
    model = _gatv2((DIM, G_HIDDEN, G_CLASSES), True, 2, True, False, HEADS, seed=5).cuda()
    logits = full_graph_inference(model, indptr, indices, feat, batch_rows=4096)
    torch.testing.assert_close(full_graph_inference(model, indptr, indices, feat, batch_rows=257), logits, rtol=1e-5,
                               atol=1e-5)
    logits = full_graph_inference(model, indptr, indices, feat)
    rng = np.random.default_rng(3)
    pred = logits.argmax(1).cpu().numpy()
    label = pred.copy()
    flip = rng.random(G_N) < 0.4
    label[flip] = rng.integers(0, G_CLASSES, size=int(flip.sum()))
    test_set = rng.permutation(G_N)[:1500].astype(np.uint32)
    want = float((pred[test_set] == label[test_set]).mean())
    accs = [train_accuracy.Accuracy((indptr, indices), test_set[:100], test_set, feat.numpy(), label.astype(np.uint64),
                                    [10, 5], 512, "cuda:0", seed=seed, exact=True).test_acc(model, "cuda:0")
            for seed in (1, 0xBEEF)]
    assert accs[0] == accs[1] == want
