"""The config key feat_store_dtype = f16 through the drop-in boundary on a real GPU (tests/f16_engine_runner.py on the
small synthetic dataset of tests/engine_runner.py): every batch's features are torch.float16 and byte-equal to
feat_f16[input_nodes], whether they come from the sampler's own gather (arch1), from the HBM cache + the host table
(arch3, cache 0.2) or from a trainer process behind the message ring (arch5, one sampler and one trainer on the one
GPU, cache 0.2); the sampled blocks are those of the run without the key."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "f16_engine_runner.py")
# two batches per epoch, one epoch: the dataset, the engine's start and the oracle's replay are the cost of a run
ENV = {"FGNN_TEST_NUM_TRAIN": "512", "FGNN_TEST_NUM_EPOCH": "1"}


def _run(tmp_path, arch, store, cache):
    work = tmp_path / store
    work.mkdir()
    out = str(work / "batches.json")
    p = subprocess.run([sys.executable, RUNNER, arch, str(work), store, str(cache), out], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **ENV))
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert "ok" in p.stdout
    return json.load(open(out))


@pytest.mark.parametrize("arch,cache", [("arch1", 0.0), ("arch3", 0.2), ("arch5", 0.2)])
def test_f16_store_returns_half_rows_and_the_same_blocks(tmp_path, arch, cache):
    half = _run(tmp_path, arch, "f16", cache)
    full = _run(tmp_path, arch, "f32", cache)
    assert len(half["digests"]) == 2 and half["digests"] == full["digests"]
    if arch == "arch3":
        assert half["miss_rows"] == full["miss_rows"] > 0
