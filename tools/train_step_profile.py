#!/usr/bin/env python3
"""Where does a training step (the layers of examples/models.py on the engine's COO blocks) spend GPU time?
Default (--model graphsage): synthetic blocks of the papers100M-shaped batch size.  --model gcn / pinsage / gat: the blocks
of one real batch of bench.py's twitter / uk-2006-05 / products workload (same graph, train set and sampler), the op-by-op and the
fused model stepped in alternation in this process (--ab alternations of --ab-steps steps, medians and spread per
model), then the per-kernel table of the --fused one.  Profiling aid."""
import argparse
import os
import sys

import torch
import torch.nn as nn
from torch.profiler import ProfilerActivity, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
from models import MODELS, SAGE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="graphsage", choices=["graphsage", "gcn", "pinsage", "gat"])
ap.add_argument("--fused", type=int, default=None, choices=[0, 1],
                help="the fused layers (1) or the op-by-op ones (0); default 1 (graphsage: SAGE_FUSED)")
ap.add_argument("--ab", type=int, default=5, help="gcn / pinsage: alternations of the op-by-op and the fused model")
ap.add_argument("--ab-steps", type=int, default=50)
ap.add_argument("--workload", default=None, help="gcn / pinsage: bench.py workload the batch comes from")
ap.add_argument("--kernel-lib", default=None, metavar="PATH",
                help="another build of libfgnn_hip.so to bind (lib.use_library), e.g. an earlier commit's: the C ABI is "
                     "the yardstick, so one Python tree times either build")
ap.add_argument("--feat-store", default="f32", choices=["f32", "f16"],
                help="f16: A/B of the fused model fed fp32 input features against the same model fed the same features "
                     "as fp16 rows (interleaved alternations in one process, median and spread of --ab), for the "
                     "layer-0 aggregation alone and for the whole step; graphsage takes the papers100M-shaped batch")
args = ap.parse_args()
if args.fused is not None:
    os.environ["SAGE_FUSED"] = str(args.fused)
if args.kernel_lib:
    from fgnn_hip import lib as _kernel_lib
    _kernel_lib.use_library(args.kernel_lib)
    print("kernel library: %s" % _kernel_lib.LIB_PATH)


def real_batch_blocks(workload, dev):
    """the COO blocks (outermost first), labels and feature width of ONE batch that bench.py's sampler draws for
    `workload`: same generated graph, train set and sampler configuration (benchlib/single.py)"""
    sys.path.insert(0, ROOT)
    from benchlib.common import SAMPLE_TYPES, WORKLOADS, gen_graph_on_gpu, gen_prefix_on_gpu, gen_train_set, lib
    w = WORKLOADS[workload]
    indptr, indices, num_edge = gen_graph_on_gpu(w["num_node"], w["num_edge"], 42, dev)
    prefix = gen_prefix_on_gpu(indptr, num_edge, 11, dev) if w["sample_type"] == "weighted_khop_prefix" else None
    sampler = lib.Sampler(indptr, indices, w["fanout"], w["batch_size"], sample_type=SAMPLE_TYPES[w["sample_type"]],
                          seed=0x5A4D47, prob_prefix=prefix, walk_len=w.get("walk_len", 3),
                          num_walks=w.get("num_walks", 4), restart_prob=w.get("restart_prob", 0.5))
    bt = sampler.new_batch()
    seeds = gen_train_set(None, w, dev)[:w["batch_size"]]
    sampler.sample(seeds, 0, bt)
    bt.finish()
    m = bt.wait()
    blocks = []
    for l in range(m.num_layers):
        row, col, nsrc, ndst = bt.graph(l)
        b = Block(row.clone(), col.clone(), nsrc, ndst)
        data = bt.graph_data(l)
        if data is not None:
            b.edata["weights"] = data.clone()
        blocks.append(b)
    blocks.sort(key=lambda b: -b.nsrc)
    assert all(a.ndst == b.nsrc for a, b in zip(blocks, blocks[1:])), [(b.nsrc, b.ndst) for b in blocks]
    del sampler, bt, indptr, indices, prefix
    torch.cuda.empty_cache()
    return blocks, w


def ab_main():
    """--model gcn / pinsage: the op-by-op model (the baseline) against the fused one, trained as benchlib/pipeline.py
    trains (fgnn_hip.nn.Adam, fgnn_softmax_xent, dropout_step set, dropout 0.5, hidden 256)"""
    import statistics
    from fgnn_hip.nn import Adam, softmax_xent
    dev = "cuda:0"
    torch.cuda.set_device(0)
    workload = args.workload or {"gcn": "twitter", "pinsage": "uk-2006-05", "gat": "products"}[args.model]
    blocks, w = real_batch_blocks(workload, dev)
    print("%s batch of %s: %s" % (args.model, workload, ", ".join(
        "%d src -> %d dst, %d edges" % (b.nsrc, b.ndst, b.row.numel()) for b in blocks)))
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(blocks[0].nsrc, w["feat_dim"], device=dev, generator=g)
    y = torch.randint(0, w["num_class"], (blocks[-1].ndst,), device=dev, generator=g)
    steppers = {}
    for fused in (0, 1):
        torch.manual_seed(0)
        model = MODELS[args.model](w["feat_dim"], 256, w["num_class"], len(blocks), 0.5, fused=bool(fused)).to(dev)
        opt = Adam(model.parameters(), lr=0.003)
        model.dropout_step = opt.step_count

        def step(model=model, opt=opt):
            out = model(blocks, x)
            loss, grad = softmax_xent(out, y)
            opt.zero_grad()
            out.backward(grad)
            opt.step()
        steppers[fused] = step
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(step, n):
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n
    for fused in (0, 1):  # warm-up: lazy initialisation, GEMM selection (_weight_grad), allocator
        run(steppers[fused], 10)
    ms = {0: [], 1: []}
    for _ in range(args.ab):
        for fused in (0, 1):
            ms[fused].append(run(steppers[fused], args.ab_steps))
    for fused in (0, 1):
        v = ms[fused]
        print("fused=%d: median %.3f ms per step, min %.3f, max %.3f, spread %.3f  (%s)"
              % (fused, statistics.median(v), min(v), max(v), max(v) - min(v), " ".join("%.3f" % t for t in v)))
    gain = statistics.median(ms[0]) - statistics.median(ms[1])
    print("op-by-op median - fused median = %.3f ms; spread of the op-by-op runs %.3f ms: %s"
          % (gain, max(ms[0]) - min(ms[0]), "ACCEPT" if gain > max(ms[0]) - min(ms[0]) else "REJECT"))
    which = 1 if args.fused is None else args.fused
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(5):
            steppers[which]()
        torch.cuda.synchronize()
    print("per-kernel times of 5 steps, fused=%d" % which)
    print(prof.key_averages().table(sort_by="self_cuda_time_total", row_limit=int(os.environ.get('ROWS', '30')),
                                    max_name_column_width=70))


class Block:
    def __init__(self, row, col, nsrc, ndst):
        self.row, self.col, self.nsrc, self.ndst = row, col, nsrc, ndst
        self.edata = {}

    def number_of_dst_nodes(self):
        return self.ndst


def feat_store_main():
    """--feat-store f16: one fused model, one batch; variant f32 reads x, variant f16 reads x.half() (no upcast pass:
    the first layer's kernels convert on load).  Timed with events around --ab-steps calls, --ab interleaved
    alternations; reports median and spread per variant and the bytes of input rows the aggregation reads."""
    import statistics
    from fgnn_hip.nn import Adam, aggregate_into, aggregate_scaled_into, block_degrees, softmax_xent
    dev = "cuda:0"
    torch.cuda.set_device(0)
    workload = args.workload or {"graphsage": "papers100M", "gcn": "twitter", "pinsage": "uk-2006-05",
                                 "gat": "products"}[args.model]
    blocks, w = real_batch_blocks(workload, dev)
    b0 = blocks[0]
    print("%s batch of %s: %s" % (args.model, workload, ", ".join(
        "%d src -> %d dst, %d edges" % (b.nsrc, b.ndst, b.row.numel()) for b in blocks)))
    g = torch.Generator(device=dev).manual_seed(0)
    x16 = torch.randn(b0.nsrc, w["feat_dim"], device=dev, generator=g).half()
    xs = {"f32": x16.float(), "f16": x16}
    y = torch.randint(0, w["num_class"], (blocks[-1].ndst,), device=dev, generator=g)
    torch.manual_seed(0)
    model = MODELS[args.model](w["feat_dim"], 256, w["num_class"], len(blocks), 0.5, fused=True).to(dev)
    opt = Adam(model.parameters(), lr=0.003)
    model.dropout_step = opt.step_count
    out0 = torch.zeros((b0.ndst, w["feat_dim"]), device=dev)
    sdeg, ddeg = block_degrees(b0.row, b0.col, b0.nsrc, b0.ndst)

    def step(x):
        out = model(blocks, x)
        loss, grad = softmax_xent(out, y)
        opt.zero_grad()
        out.backward(grad)
        opt.step()

    def aggregate(x):
        if args.model == "gcn":
            aggregate_scaled_into(out0, x, b0.row, b0.col, None, sdeg, 1, ddeg, 1)
        else:
            aggregate_into(out0, x, b0.row, b0.col)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(fn, x, n):
        e0.record()
        for _ in range(n):
            fn(x)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n
    touched = int(torch.unique(b0.row).numel())
    for what, fn in (("layer-0 aggregation", aggregate), ("whole step", step)):
        for k in xs:
            run(fn, xs[k], 10)
        ms = {k: [] for k in xs}
        for _ in range(args.ab):
            for k in xs:
                ms[k].append(run(fn, xs[k], args.ab_steps))
        for k, v in ms.items():
            print("%s, %s rows: median %.4f ms, min %.4f, max %.4f, spread %.4f  (%s)"
                  % (what, k, statistics.median(v), min(v), max(v), max(v) - min(v), " ".join("%.4f" % t for t in v)))
        gain = statistics.median(ms["f32"]) - statistics.median(ms["f16"])
        spread = max(max(v) - min(v) for v in ms.values())
        print("%s: f32 median - f16 median = %.4f ms, larger spread %.4f ms: f16 %s" % (
            what, gain, spread, "FASTER" if gain > spread else "NOT FASTER beyond the spread"))
    print("input rows read per aggregation: %d edges x %d B (f32) / %d B (f16) = %.1f / %.1f MB; distinct source rows "
          "%d = %.1f / %.1f MB" % (b0.row.numel(), 4 * w["feat_dim"], 2 * w["feat_dim"],
                                   b0.row.numel() * 4e-6 * w["feat_dim"], b0.row.numel() * 2e-6 * w["feat_dim"], touched,
                                   touched * 4e-6 * w["feat_dim"], touched * 2e-6 * w["feat_dim"]))


if args.feat_store == "f16":
    feat_store_main()
    sys.exit(0)
if args.model != "graphsage":
    ab_main()
    sys.exit(0)

dev = "cuda:0"
g = torch.Generator(device=dev)
g.manual_seed(0)
# the papers100M-shaped R-MAT batch of bench.py: layer 0 (outer) 302 K src -> 22.5 K dst, 371 K edges; layer 1: 22.5 K src
# -> 8000 dst, 15 K edges
S0, D0, E0, E1 = 302000, 22500, 371000, 15000
b0 = Block(torch.randint(0, S0, (E0,), device=dev, generator=g, dtype=torch.int32), torch.sort(torch.randint(0, D0, (E0,), device=dev, generator=g, dtype=torch.int32))[0], S0, D0)
b1 = Block(torch.randint(0, D0, (E1,), device=dev, generator=g, dtype=torch.int32), torch.sort(torch.randint(0, 8000, (E1,), device=dev, generator=g, dtype=torch.int32))[0], D0, 8000)
x = torch.randn(S0, 128, device=dev)
y = torch.randint(0, 172, (8000,), device=dev)
model = SAGE(128, 256, 172, 2, 0.5, fused=os.environ.get('SAGE_FUSED', '1') == '1').to(dev)
# TRAIN_OPS=1 (default): the one-launch pieces of csrc/train_ops.hip as bench.py's train legs use them (fgnn_hip.nn.Adam,
# fused ReLU + dropout keyed by its step count, fgnn_softmax_xent); 0: torch's fused Adam, F.relu + Dropout, CrossEntropyLoss
TRAIN_OPS = os.environ.get('TRAIN_OPS', '1') == '1'
lossf = nn.CrossEntropyLoss()
if TRAIN_OPS:
    from fgnn_hip.nn import Adam, softmax_xent
    opt = Adam(model.parameters(), lr=0.003)
    model.dropout_step = opt.step_count
else:
    opt = torch.optim.Adam(model.parameters(), lr=0.003, fused=os.environ.get('ADAM_FUSED', '1') == '1', capturable=True)


def step():
    out = model([b0, b1], x)
    if TRAIN_OPS:
        loss, g = softmax_xent(out, y)
        opt.zero_grad()
        out.backward(g)
    else:
        loss = lossf(out, y)
        opt.zero_grad()
        loss.backward()
    opt.step()


for _ in range(5):
    step()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    step()
e1.record()
torch.cuda.synchronize()
print("eager step %.3f ms (SAGE_FUSED=%s TRAIN_OPS=%s)" % (e0.elapsed_time(e1) / 20, os.environ.get('SAGE_FUSED', '1'), TRAIN_OPS))
# the same step replayed as a captured graph (what examples/graphed_step.py does per size bucket)
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(3):
        graph.replay()
    side.synchronize()
    e0.record()
    for _ in range(20):
        graph.replay()
    e1.record()
    side.synchronize()
    print("graph replay %.3f ms per step" % (e0.elapsed_time(e1) / 20))
    with profile(activities=[ProfilerActivity.CUDA]) as gprof:
        for _ in range(5):
            graph.replay()
        side.synchronize()
    rows = [(e.key, e.count, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total)
            for e in gprof.key_averages()]
    rows.sort(key=lambda r: -r[2])
    nk = sum(r[1] for r in rows) / 5
    print("graph: %.0f kernel / memset nodes per step, %.0f us of device time per step" % (nk, sum(r[2] for r in rows) / 5))
    for k, c, t in rows[:40]:
        print("  %-90s x%-3d %8.1f us per step" % (k[:90], c // 5, t / 5))
torch.cuda.current_stream().wait_stream(side)
if os.environ.get("GRAPH_ONLY"):
    sys.exit(0)
# weight-gradient GEMM gy^T x at the row counts a batch's layers have: library GEMM against the 32-slice batched GEMM
for m in (8000, 22500, 88000, 302000):
    for (k, n) in ((128, 256), (256, 172)):
        xx, gy = torch.randn(m, k, device=dev), torch.randn(m, n, device=dev)
        mp = m // 32 * 32

        def t(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / 10 * 1e3
        a = t(lambda: gy.t().mm(xx))
        b = t(lambda: torch.bmm(gy[:mp].view(32, mp // 32, -1).transpose(1, 2), xx[:mp].view(32, mp // 32, -1)).sum(0))
        print("gw %6d x %3d x %3d: mm %.1f us, 32-slice bmm + sum %.1f us" % (m, k, n, a, b))
with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
    for _ in range(5):
        step()
    torch.cuda.synchronize()
print(prof.key_averages().table(sort_by="self_cuda_time_total", row_limit=int(os.environ.get('ROWS', '30')), max_name_column_width=70))
