#!/usr/bin/env python3
"""How many rows does a batch move when the seeds of a layer share one random key per node (sample type khop_shared,
csrc/sample_khop_shared.hip) instead of drawing independently (khop0, khop2)?  The bench's papers100M-shaped R-MAT graph
(fgnn_hip.rmat, seed 42), batch 8000, fanout [25, 10]; the SAME seed batches go through the batch driver (fgnn_sampler)
with each of the three samplers.  Reported per sampler: mean num_input and num_src per layer, the bytes a D = 128 fp32
feature gather moves for them, and ms per batch for sampling alone and for sampling + cache-less feature gather --
batches one after the other on one stream (a latency, not the pipelined throughput bench.py reports), interleaved
alternations of the three in one process, median and spread of --ab rounds of --steps batches each.  No ratio is fixed
in advance: the verdict is printed as it comes out.
usage: khop_shared_ab.py [--num-node N] [--num-edge E] [--batches 32] [--ab 7] [--steps 16]
                         [--out profiles/r15_a_khop_shared_ab.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
from fgnn_hip import lib, rmat, synth  # noqa: E402

shape = synth.DATASET_SHAPES["papers100M"]
ap = argparse.ArgumentParser()
ap.add_argument("--num-node", type=int, default=shape["num_node"])
ap.add_argument("--num-edge", type=int, default=shape["num_edge"])
ap.add_argument("--batches", type=int, default=32, help="seed batches the row counts are averaged over")
ap.add_argument("--ab", type=int, default=7)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_a_khop_shared_ab.txt"))
args = ap.parse_args()
FANOUT, BATCH, DIM, SEED = [25, 10], 8000, 128, 0x5A4D47
lib.load()
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


indptr, indices, E = rmat.rmat_csr(args.num_node, args.num_edge, seed=42, device=dev)
N = args.num_node
deg = (indptr[1:].long() & 0xFFFFFFFF) - (indptr[:-1].long() & 0xFFFFFFFF)
p = lib.khop_shared_params()
say("R-MAT (fgnn_hip.rmat, seed 42): %d nodes, %d edges; longest row %d; rows above the wave / workgroup / hub lengths "
    "(%d / %d / %d): %d / %d / %d" % (N, E, int(deg.max()), 64, p["wave_row"], p["block_row"], int((deg > 64).sum()),
                                     int((deg > p["wave_row"]).sum()), int((deg > p["block_row"]).sum())))
del deg
train = rmat.train_set(N, max(args.batches, args.steps) * BATCH, 1, dev)
feat = torch.empty((N, DIM), dtype=torch.float32, device=dev)
for a in range(0, N, 1 << 24):  # contents do not matter to the gather
    feat[a:a + (1 << 24)].fill_(1.0)
label = torch.zeros(N, dtype=torch.int64, device=dev)
KINDS = {"khop0": lib.KHOP0, "khop2": lib.KHOP2, "khop_shared": lib.KHOP_SHARED}
samplers, batches, seqs = {}, {}, {}
for name, st in KINDS.items():
    own = indices.clone() if st == lib.KHOP2 else indices  # khop2 swaps the entries of the rows it draws from
    samplers[name] = lib.Sampler(indptr, own, FANOUT, BATCH, sample_type=st, seed=SEED)
    batches[name] = samplers[name].new_batch(DIM, lib.F32, lib.I64)
    seqs[name] = 0


def one(name, b, gather):
    seeds = train[b * BATCH:(b + 1) * BATCH]
    s, bt = samplers[name], batches[name]
    if gather:
        s.run_batch(seqs[name], seeds, b, bt, None, feat, label)
    else:
        s.sample(seeds, b, bt, seq=seqs[name])
        bt.finish()
    seqs[name] += 1


rows = {}
for name in KINDS:
    tot = {"num_input": 0, "num_src1": 0, "num_src0": 0, "num_edge1": 0, "num_edge0": 0}
    for b in range(args.batches):
        one(name, b, False)
        m = batches[name].wait()
        tot["num_input"] += m.num_input
        for l in (0, 1):
            tot["num_src%d" % l] += m.num_src[l]
            tot["num_edge%d" % l] += m.num_edge[l]
    rows[name] = {k: v / args.batches for k, v in tot.items()}
    r = rows[name]
    say("%-11s mean over %d batches: num_input %.0f (gather of %d x fp32: %.1f MB); layer 1 (seeds, fanout %d): %.0f edges,"
        " num_src %.0f; layer 0 (fanout %d): %.0f edges, num_src %.0f"
        % (name, args.batches, r["num_input"], DIM, r["num_input"] * DIM * 4 / 1e6, FANOUT[1], r["num_edge1"], r["num_src1"],
           FANOUT[0], r["num_edge0"], r["num_src0"]))
for base in ("khop0", "khop2"):
    say("khop_shared / %s: num_input x %.3f, layer-1 num_src x %.3f"
        % (base, rows["khop_shared"]["num_input"] / rows[base]["num_input"],
           rows["khop_shared"]["num_src1"] / rows[base]["num_src1"]))

e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def run(name, gather):
    e0.record()
    for b in range(args.steps):
        one(name, b, gather)
    e1.record()
    e1.synchronize()
    batches[name].wait()
    return e0.elapsed_time(e1) / args.steps


ms = {(name, g): [] for name in KINDS for g in (False, True)}
for key in ms:
    run(*key)  # warm-up of every shape
for _ in range(args.ab):
    for key in ms:
        ms[key].append(run(*key))
med = {k: statistics.median(v) for k, v in ms.items()}
for (name, g), v in ms.items():
    say("%-11s %-15s median %.4f ms per batch, min %.4f, max %.4f, spread %.4f  (%s)"
        % (name, "sample + gather" if g else "sample", med[name, g], min(v), max(v), max(v) - min(v),
           " ".join("%.4f" % t for t in v)))
for g in (False, True):
    for base in ("khop0", "khop2"):
        spread = max(max(ms[n, g]) - min(ms[n, g]) for n in (base, "khop_shared"))
        diff = med["khop_shared", g] - med[base, g]
        verdict = ("NO DIFFERENCE beyond the spread" if abs(diff) <= spread else
                   "khop_shared SLOWER by more than the spread" if diff > 0 else
                   "khop_shared FASTER by more than the spread")
        say("%s: khop_shared - %s = %+.4f ms (x %.2f; the larger spread of the two %.4f): %s"
            % ("sample + gather" if g else "sample", base, diff, med["khop_shared", g] / med[base, g], spread, verdict))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
