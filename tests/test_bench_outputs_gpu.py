"""bench.py --gpus 1 as every later change is measured: a plain run does the headline only (what else the benchmark
measures is behind --full) and --dump-outputs writes the last timed step's batch -- the arrays a caller of the timed
path receives -- so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, WINDOWS = 6, 2, 5
FEAT_ROWS = (24 << 20) // (128 * 4)  # rows of the feature sample (benchlib/single.py: dump_batch)


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_dump")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "small", "--steps",
                        str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(d / "out")], capture_output=True,
                       text=True, timeout=300, env=env, cwd=str(d))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return line, {f[:-4]: np.load(str(d / "out" / f)) for f in sorted(os.listdir(str(d / "out")))}


@pytest.mark.gpu
def test_plain_run_measures_the_headline_only(plain_run):
    line, _ = plain_run
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # ms_per_step is the median window's seconds per step, value that window's edges per second
    wd = line["windows"]
    assert wd["count"] == WINDOWS and line["ms_per_step"] == sorted(wd["ms_per_step"])[(WINDOWS - 1) // 2]
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / line["edges_per_step"] - 1) < 1e-9
    for k in ("sample_stage", "roofline_extract", "train_leg", "roofline_sample", "probe_random_reads_per_s",
              "pipeline_n1_point"):
        assert line[k] is None, k
    assert "cpu_baseline" not in line and line["roofline"]["torch_copy_GBps"] is None and line["roofline"]["serial"] is None
    assert 0 < line["roofline"]["frac"] < 1  # the gather's figure comes from events inside the timed windows


@pytest.mark.gpu
def test_dumped_outputs_are_the_last_timed_batch(plain_run):
    import torch
    import bench
    line, out = plain_run
    w = bench.WORKLOADS["small"]
    L, bs, dim = len(w["fanout"]), w["batch_size"], w["feat_dim"]
    names = {"input_nodes", "output_nodes", "label", "feat", "miss_src_index", "miss_dst_index", "cache_src_index",
             "cache_dst_index"} | {"layer%d_%s" % (l, k) for l in range(L) for k in ("row", "col", "num_src_dst")}
    assert set(out) == names
    assert all(a.dtype == (np.float32 if n == "feat" else np.float64) for n, a in out.items())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    # the seeds of the last timed step: the same train set, the same slice, whichever build runs the benchmark
    last = max(0, 12 - WARMUP) + WARMUP + WINDOWS * STEPS - 1
    steps_per_epoch = (w["num_train"] + bs - 1) // bs
    step = last % steps_per_epoch
    train = bench.gen_train_set(None, w, torch.device("cuda", 0))
    seeds = train[step * bs:(step + 1) * bs].cpu().numpy().view(np.uint32).astype(np.float64)
    np.testing.assert_array_equal(out["output_nodes"], seeds)
    # an array longer than its share of the 64 MB holds a fixed sample of its rows (dump_batch): the positions kept
    cap = ((60 << 20) - (24 << 20)) // (3 * L + 7) // 8

    def kept(n, rows):
        return np.arange(n) if n <= rows else np.sort(np.random.default_rng(n).choice(n, size=rows, replace=False))
    n_out = len(seeds)
    n_in = int(out["layer0_num_src_dst"][0])
    nodes, pos = out["input_nodes"], kept(n_in, cap)
    assert len(nodes) == len(pos) and len(np.unique(nodes)) == len(nodes) and nodes.max() < w["num_node"]

    def node_at(q):
        """(mask of the positions q whose node id was written, those ids)"""
        m = np.isin(q, pos)
        return m, nodes[np.searchsorted(pos, q[m])]
    m, got = node_at(np.arange(n_out))
    assert m.any()
    np.testing.assert_array_equal(got, seeds[m])  # the unique list starts with the seeds
    assert out["layer%d_num_src_dst" % (L - 1)][1] == n_out
    for l in range(L - 1):
        assert out["layer%d_num_src_dst" % l][1] == out["layer%d_num_src_dst" % (l + 1)][0]
    for l in range(L):
        nsrc, ndst = out["layer%d_num_src_dst" % l]
        row, col = out["layer%d_row" % l], out["layer%d_col" % l]
        assert len(row) == len(col) > 0 and row.max() < nsrc and col.max() < ndst
    assert abs(n_in - line["input_nodes_per_step"]) < 0.2 * n_in
    # cache-index split: an input position is a miss or a hit, never both; a miss carries its node id
    md, cd = out["miss_dst_index"].astype(np.int64), out["cache_dst_index"].astype(np.int64)
    assert len(np.unique(md)) == len(md) and len(np.unique(cd)) == len(cd) and not np.isin(md, cd).any()
    assert max(md.max(), cd.max()) < n_in and len(out["miss_src_index"]) == len(md) and len(out["cache_src_index"]) == len(cd)
    if len(md) < cap and len(cd) < cap:  # both written whole: together they are every input position
        np.testing.assert_array_equal(np.sort(np.concatenate([md, cd])), np.arange(n_in))
    m, got = node_at(md)
    assert m.any()
    np.testing.assert_array_equal(out["miss_src_index"][m], got)
    assert out["cache_src_index"].max() < int(w["num_node"] * 0.2)  # rows of the cache (default ratio 0.2)
    assert out["label"].shape == (n_out,) and out["label"].min() >= 0 and out["label"].max() < w["num_class"]
    # features: the rows of the synthetic table for the (sampled) input positions, bit for bit
    rows = kept(n_in, FEAT_ROWS)
    assert out["feat"].shape == (len(rows), dim)
    m, ids = node_at(rows)
    assert m.sum() > 1000
    ids = ids.astype(np.int64)
    want = (((ids[:, None] * 131 + np.arange(dim)[None, :] * 7) & 0xFFFF).astype(np.float32) * np.float32(1.0 / 65536.0))
    np.testing.assert_array_equal(out["feat"][m], want)
