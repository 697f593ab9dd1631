#!/usr/bin/env python3
"""One engine run on the small synthetic dataset of tests/engine_runner.py (helpers imported from there) with the
config key feat_store_dtype set to f16, or left out (the f32 default): every batch's blocks are checked against the
oracle, its features against the rows of the table the key selects, byte for byte, and a digest of every batch's
blocks goes to a JSON file for the test to compare the two runs by.  Run as a subprocess by
tests/test_f16_engine_gpu.py (the engine is a process-wide singleton).

usage: f16_engine_runner.py <arch1|arch3|arch5> <workdir> <f32|f16> <cache_pct> <out.json>"""
import hashlib
import json
import multiprocessing as mp
import os
import sys
import traceback

import numpy as np

import engine_runner as E

SAMPLE_TYPE = "khop2"


def prepare(workdir, store):
    """(path, table, labels): the dataset, feat_f16.bin beside feat.bin for the f16 run, the table a batch's features
    must be rows of, and the label file"""
    path = E.dataset(workdir, SAMPLE_TYPE)
    feat = np.fromfile(os.path.join(path, "feat.bin"), dtype=np.float32).reshape(E.NUM_NODE, E.DIM)
    if store == "f16":
        feat = feat.astype(np.float16)
        feat.tofile(os.path.join(path, "feat_f16.bin"))
    return path, feat, np.fromfile(os.path.join(path, "label.bin"), dtype=np.int64)


def config(path, arch, store, **more):
    cfg = E.base_config(path, arch, SAMPLE_TYPE)
    cfg.update(more)
    if store == "f16":
        cfg["feat_store_dtype"] = "f16"
    return cfg


def check(sam, key, seeds, task, table, labels, digests):
    import torch
    nl = len(task["graphs"])
    blocks, feat, label = sam.get_dgl_blocks(key, nl, True)
    h = hashlib.sha1()
    for li in range(nl):
        row = blocks[li].row.cpu().numpy().view(np.uint32)
        col = blocks[li].col.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(row, task["graphs"][li]["row"])
        np.testing.assert_array_equal(col, task["graphs"][li]["col"])
        h.update(row.tobytes())
        h.update(col.tobytes())
    want = torch.float16 if table.dtype == np.float16 else torch.float32
    assert feat.dtype == want, "key %d: features are %s, the store is %s" % (key, feat.dtype, table.dtype)
    assert tuple(feat.shape) == (len(task["input_nodes"]), E.DIM)
    assert feat.cpu().numpy().tobytes() == table[task["input_nodes"]].tobytes(), "key %d feat" % key
    np.testing.assert_array_equal(label.cpu().numpy(), labels[seeds])
    from samgraph.torch import c_lib
    f2 = c_lib.samgraph_torch_get_graph_feat(key)
    assert f2.dtype == want and f2.data_ptr() == feat.data_ptr()
    digests[str(key)] = h.hexdigest()


def run_inproc(arch, workdir, store, cache_pct, out):
    import torch
    path, table, labels = prepare(workdir, store)
    import samgraph.torch as sam
    cfg = config(path, {"arch1": sam.kArch1, "arch3": sam.kArch3}[arch], store, sampler_ctx="cuda:0",
                 trainer_ctx="cuda:0", cache_percentage=cache_pct)
    sam.config(cfg)
    sam.init()
    rep = E.OracleReplay(path, SAMPLE_TYPE, 0, 1, arch != "arch1" and cache_pct > 0)
    assert sam.get_dataset_feat().dtype == (torch.float16 if store == "f16" else torch.float32)
    digests, misses = {}, 0
    for key, seeds, task in rep.epochs():
        sam.sample_once()
        assert sam.get_next_batch() == key
        check(sam, key, seeds, task, table, labels, digests)
        if arch != "arch1" and cache_pct > 0:  # the miss volume is counted in bytes of the store's rows
            cached = np.zeros(E.NUM_NODE, dtype=bool)
            cached[rep.rank[:int(E.NUM_NODE * cache_pct)]] = True
            m = int((~cached[task["input_nodes"]]).sum())
            epoch, step = key // rep.num_step, key % rep.num_step
            assert sam.get_log_step_value(epoch, step, sam.kLogL1MissBytes) == m * E.DIM * table.itemsize
            misses += m
    sam.shutdown()
    json.dump({"digests": digests, "miss_rows": misses}, open(out, "w"))


def _trainer(path, table, labels, cache_pct, barrier, err, out):
    try:
        import samgraph.torch as sam
        barrier.wait()
        sam.train_init(0, E.TRAINER_DEV)
        rep = E.OracleReplay(path, SAMPLE_TYPE, 0, 1, cache_pct > 0)
        expected = {key: (seeds, task) for key, seeds, task in rep.epochs()}
        sam.extract_start(len(expected))
        digests = {}
        for _ in range(len(expected)):
            key = sam.get_next_batch()
            seeds, task = expected.pop(key)
            check(sam, key, seeds, task, table, labels, digests)
        sam.shutdown()
        json.dump({"digests": digests}, open(out, "w"))
    except BaseException:
        traceback.print_exc()
        err.value = 1
        os._exit(1)


def run_arch5(workdir, store, cache_pct, out):
    """one sampler and one trainer process on the one GPU, forked like the reference's multi_gpu scripts"""
    path, table, labels = prepare(workdir, store)
    import samgraph.torch as sam
    sam.config(config(path, sam.kArch5, store, num_sample_worker=1, num_train_worker=1, cache_percentage=cache_pct))
    sam.data_init()
    ctx = mp.get_context("fork")
    barrier, err = ctx.Barrier(2), ctx.Value("i", 0)
    procs = [ctx.Process(target=E._sampler_proc, args=(0, 1, barrier, err)),
             ctx.Process(target=_trainer, args=(path, table, labels, cache_pct, barrier, err, out))]
    for p in procs:
        p.start()
    if E._join_all(procs, ["sampler", "trainer"]) or err.value:
        sys.exit(1)


if __name__ == "__main__":
    arch, workdir, store, cache_pct, out = sys.argv[1], sys.argv[2], sys.argv[3], float(sys.argv[4]), sys.argv[5]
    assert store in ("f32", "f16")
    if arch == "arch5":
        run_arch5(workdir, store, cache_pct, out)
    else:
        run_inproc(arch, workdir, store, cache_pct, out)
    print("%s %s cache %.2f ok" % (arch, store, cache_pct))
