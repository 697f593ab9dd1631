"""arch1 batches of the engine with sample type khop_shared (a subprocess of tests/test_khop_shared_gpu.py)."""
import os
import sys

import numpy as np

import engine_runner as er  # puts the package on the path; dataset and run configuration of the other engine tests
import khop_shared_refs as refs
import samgraph.torch as sam

path = er.dataset(sys.argv[1], "khop0")
cfg = er.base_config(path, sam.kArch1, "khop0")
cfg.update(_sample_type=sam.all_sample_types["khop_shared"], sampler_ctx="cuda:0", trainer_ctx="cuda:0")
sam.config(cfg)
sam.init()
indptr = np.fromfile(os.path.join(path, "indptr.bin"), dtype=np.uint32)
indices = np.fromfile(os.path.join(path, "indices.bin"), dtype=np.uint32)
fanouts = cfg["fanout"]
u32 = (lambda t: t.cpu().numpy().view(np.uint32))
for _ in range(6):
    sam.sample_once()
    key = sam.get_next_batch()
    blocks, feat, label = sam.get_dgl_blocks(key, len(fanouts), True)
    graphs = [(u32(b.row), u32(b.col), sam.get_graph_num_src(key, l), sam.get_graph_num_dst(key, l))
              for l, b in enumerate(blocks)]
    input_nodes, seeds = u32(sam.get_graph_input_nodes(key)), u32(sam.get_graph_output_nodes(key))
    assert len(seeds) == er.BATCH and tuple(feat.shape) == (len(input_nodes), er.DIM)
    refs.check_batch(indptr, indices, input_nodes, graphs, fanouts, seeds, er.SEED, key)
sam.shutdown()
print("khop_shared arch1 ok")
