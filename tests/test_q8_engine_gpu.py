"""The config value feat_store_dtype = q8 through the drop-in boundary on a real GPU: the first batch of the small
synthetic dataset of tests/engine_runner.py (arch3: the trainer-side extraction from the HBM cache and the host table)
carries a [num_input, S] uint8 tensor whose rows are rows input_nodes of feat_q8.bin, byte for byte, and the blocks and
input nodes of the run without the key.  One child process per run: the engine is a process-wide singleton."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ENV = {"FGNN_TEST_NUM_TRAIN": "512", "FGNN_TEST_NUM_EPOCH": "1"}
SCRIPT = """
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, %r)
import engine_runner as E, q8_refs as Q
work, store, cache = sys.argv[1], sys.argv[2], float(sys.argv[3])
path = E.dataset(work, "khop2")
feat = np.fromfile(os.path.join(path, "feat.bin"), dtype=np.float32).reshape(E.NUM_NODE, E.DIM)
table = Q.encode(feat)
table.tofile(os.path.join(path, "feat_q8.bin"))
import torch
import samgraph.torch as sam
from samgraph.torch import c_lib
cfg = E.base_config(path, sam.kArch3, "khop2")
cfg.update(sampler_ctx="cuda:0", trainer_ctx="cuda:0", cache_percentage=cache)
if store == "q8":
    cfg["feat_store_dtype"] = "q8"
sam.config(cfg)
sam.init()
assert sam.feat_dim() == E.DIM
sam.sample_once()
key = sam.get_next_batch()
blocks, x, _ = sam.get_dgl_blocks(key, len(cfg["fanout"]), True)
# the batch's input nodes: the oracle's replay (with a cache the engine ships the cache index lists, not the node list)
_, _, task = next(iter(E.OracleReplay(path, "khop2", 0, 1, cache > 0).epochs()))
nodes = np.asarray(task["input_nodes"], dtype=np.uint32)
shipped = c_lib.samgraph_torch_get_graph_input_nodes(key).cpu().numpy().view(np.uint32)
assert shipped.size == 0 or np.array_equal(shipped, nodes)
h = hashlib.sha1(nodes.tobytes())
for b in blocks:
    h.update(b.row.cpu().numpy().tobytes() + b.col.cpu().numpy().tobytes())
if store == "q8":
    assert x.dtype == torch.uint8 and tuple(x.shape) == (len(nodes), Q.row_bytes(E.DIM)), (x.dtype, x.shape)
    assert x.cpu().numpy().tobytes() == table[nodes].tobytes()
else:
    assert x.dtype == torch.float32 and x.cpu().numpy().tobytes() == feat[nodes].tobytes()
sam.shutdown()
print("DIGEST", h.hexdigest(), len(nodes))
""" % HERE


@pytest.mark.parametrize("cache", [0.0, 0.2])
def test_q8_store_hands_the_trainer_the_files_rows_and_the_same_blocks(tmp_path, cache):
    digests = []
    for store in ("q8", "f32"):
        work = tmp_path / store
        work.mkdir()
        p = subprocess.run([sys.executable, "-c", SCRIPT, str(work), store, str(cache)], capture_output=True, text=True,
                           timeout=300, env=dict(os.environ, **ENV))
        assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-5000:]
        digests.append([ln for ln in p.stdout.splitlines() if ln.startswith("DIGEST")])
    assert digests[0] and digests[0] == digests[1]
