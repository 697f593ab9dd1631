"""examples/inference.py's gat_layerwise_inference on the GPU (attention by fgnn_csr_gat_attention) on the R-MAT graph of
tests/test_layerwise_inference_gpu.py -- about 4000 nodes, one planted hub row of 1.5 split lengths -- for GAT models of
8 heads x 8 features with 1 and 2 output heads, fused and op-by-op layers, with and without residual: against the
model's own forward on "full" blocks on the GPU and against the float64 op-by-op pass on the CPU, both within rtol 1e-4
/ atol 1e-4 (that file's tolerances for these comparisons); chunk sizes; and the paths --exact-eval and
--save-predictions take (Accuracy(exact=True), full_graph_inference), called directly: the training script keeps no
checkpoint a child process's predictions could be compared with."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from test_layerwise_inference_host import full_blocks  # noqa: E402

pytestmark = pytest.mark.gpu
N, E, DIM, HIDDEN, HEADS, CLASSES, HUB_NODE = 4000, 60000, 100, 64, 8, 7, 1234


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
    feat = torch.from_numpy(np.random.default_rng(DIM).standard_normal((N, DIM)).astype(np.float32))
    return indptr.astype(np.uint32), indices, feat


def _model(fused, out_heads, residual=False, seed=1):
    from models import GAT
    torch.manual_seed(seed)
    model = GAT(DIM, HIDDEN, CLASSES, 2, 0.5, fused=fused, heads=HEADS, out_heads=out_heads, residual=residual)
    with torch.no_grad():
        for layer in model.layers:
            layer.bias.normal_()
    return model


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("out_heads", [1, 2])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
def test_equals_the_full_block_forward_and_the_float64_pass(graph, fused, out_heads, residual):
    from inference import gat_layerwise_inference
    indptr, indices, feat = graph
    model = _model(fused, out_heads, residual).cuda()
    model.train()
    got = gat_layerwise_inference(model, indptr, indices, feat)
    assert model.training and got.is_cuda and got.shape == (N, CLASSES) and got.dtype == torch.float32
    model.eval()
    with torch.no_grad():
        want = model(full_blocks(indptr, indices, 2, device="cuda"), feat.cuda())
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    ref = gat_layerwise_inference(_model(fused, out_heads, residual).double(), indptr, indices, feat.double())
    assert ref.dtype == torch.float64 and not ref.is_cuda
    torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_chunk_size_does_not_matter(graph):
    """batch_rows 257 and 4096 within rtol 1e-5 (atol 1e-5): the attention is bitwise the same, the GEMMs may pick
    different kernels"""
    from inference import gat_layerwise_inference
    indptr, indices, feat = graph
    model = _model(True, 2, True).cuda()
    a = gat_layerwise_inference(model, indptr, indices, feat, batch_rows=257)
    b = gat_layerwise_inference(model, indptr, indices, feat, batch_rows=4096)
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


def test_half_features_are_upcast_per_chunk(graph):
    from inference import gat_layerwise_inference
    indptr, indices, feat = graph
    model = _model(True, 1).cuda()
    half = feat.half()
    assert torch.equal(gat_layerwise_inference(model, indptr, indices, half.cuda(), batch_rows=1000),
                       gat_layerwise_inference(model, indptr, indices, half.float().cuda(), batch_rows=1000))


def test_exact_eval_and_saved_predictions_take_a_gat_model(graph):
    """what train_graphsage.py --model gat --exact-eval --save-predictions runs: full_graph_inference is
    gat_layerwise_inference bit for bit, and Accuracy(exact=True) is the accuracy of its argmax whatever the seed"""
    import train_accuracy
    from inference import full_graph_inference, gat_layerwise_inference
    indptr, indices, feat = graph
    model = _model(True, 1, seed=5).cuda()
    logits = gat_layerwise_inference(model, indptr, indices, feat)
    assert torch.equal(full_graph_inference(model, indptr, indices, feat), logits)
    rng = np.random.default_rng(3)
    label = logits.argmax(1).cpu().numpy().copy()
    flip = rng.random(N) < 0.4
    label[flip] = rng.integers(0, CLASSES, size=int(flip.sum()))
    test_set = rng.permutation(N)[:1500].astype(np.uint32)
    want = float((logits.argmax(1).cpu().numpy()[test_set] == label[test_set]).mean())
    assert 0.5 < want < 0.9
    accs = []
    for seed in (1, 0xBEEF):
        acc = train_accuracy.Accuracy((indptr, indices), test_set[:100], test_set, feat.numpy(),
                                      label.astype(np.uint64), [10, 5], 512, "cuda:0", seed=seed, exact=True)
        assert not hasattr(acc, "sampler")
        accs.append(acc.test_acc(model, "cuda:0"))
    assert accs[0] == accs[1] == want
