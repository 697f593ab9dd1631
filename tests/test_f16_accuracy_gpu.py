"""A model trained through the drop-in boundary on an fp16 feature store learns what it learns on the fp32 store: the
flags of tests/test_examples_accuracy_gpu.py with --feat-store f16, fused SAGE on arch1, against the f32 run made in the
same test (that test's 0.08 between two runs)."""
import os
import sys

import pytest

import test_examples_accuracy_gpu as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    sys.path.insert(0, os.path.join(A.ROOT, "fgnn-artifacts_amd"))
    from fgnn_hip import synth
    sh = synth.LEARNABLE_SHAPE
    return synth.write_dataset(str(tmp_path_factory.mktemp("acc16")), "learn", sh["num_node"], sh["num_edge"],
                               sh["feat_dim"], sh["num_class"], sh["num_train"], sh["num_valid"], sh["num_test"],
                               learnable=True, feat_f16=True)


def test_arch1_fused_sage_learns_alike_on_half_and_full_precision_features(dataset):
    assert os.path.exists(os.path.join(dataset, "feat_f16.bin"))
    valid_h, test_h = A._run("train_graphsage.py", dataset, "--arch", "arch1", "--feat-store", "f16")
    valid_f, test_f = A._run("train_graphsage.py", dataset, "--arch", "arch1")
    print("test accuracy: f16 store %.4f, f32 store %.4f; last validation accuracy %.4f / %.4f"
          % (test_h, test_f, valid_h[-1], valid_f[-1]))
    for valid, test in ((valid_h, test_h), (valid_f, test_f)):
        assert len(valid) >= 3 and valid[-1] > 4 * A.CHANCE and test > 4 * A.CHANCE, (valid, test)
    assert abs(test_h - test_f) < 0.08, (test_h, test_f)
