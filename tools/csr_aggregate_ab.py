#!/usr/bin/env python3
"""The CSR aggregation kernel of exact layer-wise inference (fgnn_csr_aggregate: one wave per CSR row, no atomics, out
overwritten) against the sampled-block aggregation on the identical edge set expanded to COO (fgnn_block_aggregate_ex
plus the zero fill of its output: float atomics into zeros, a destination id per edge), over ALL rows of an R-MAT graph
from the bench's generator (fgnn_hip.rmat, seed 42) at the bench graph's average degree, for dims 128 and 256.
Interleaved alternations of the two in one process, median and spread of --ab rounds of --steps launches each; bytes
counted as E x row bytes read and rows x dim x 4 written.  The outputs of the two are compared first.
usage: csr_aggregate_ab.py [--num-node 4000000] [--num-edge 58000000] [--dims 128 256] [--ab 7] [--steps 20]
                           [--out profiles/r11_a_csr_aggregate_ab.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
from fgnn_hip import lib, nn, rmat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--num-node", type=int, default=4_000_000)
ap.add_argument("--num-edge", type=int, default=58_000_000, help="default: papers100M's 14.5 edges per node")
ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
ap.add_argument("--ab", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_a_csr_aggregate_ab.txt"))
args = ap.parse_args()
lib.load()
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


indptr, indices, E = rmat.rmat_csr(args.num_node, args.num_edge, seed=42, device=dev)
N = args.num_node
deg = (indptr[1:].long() & 0xFFFFFFFF) - (indptr[:-1].long() & 0xFFFFFFFF)
col = torch.repeat_interleave(torch.arange(N, device=dev, dtype=torch.int32), deg)  # the COO's destination per edge
split = nn.csr_split_length()
say("R-MAT (fgnn_hip.rmat, seed 42): %d nodes, %d edges; longest row %d, %d rows above the split length %d; the COO "
    "baseline reads %.0f MB of destination ids on top" % (N, E, int(deg.max()), int((deg > split).sum()), split,
                                                          4 * E / 1e6))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for dim in args.dims:
    h = torch.empty((N, dim), dtype=torch.float32, device=dev).normal_()
    outs = {"csr": torch.empty((N, dim), dtype=torch.float32, device=dev),
            "coo": torch.empty((N, dim), dtype=torch.float32, device=dev)}

    def launch(name):
        if name == "csr":
            nn.csr_aggregate_into(outs["csr"], h, indptr, indices)
        else:
            outs["coo"].zero_()
            nn.aggregate_into(outs["coo"], h, indices, col)

    def run(name, n):
        e0.record()
        for _ in range(n):
            launch(name)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    for name in outs:
        run(name, 3)
    scale = float(outs["coo"].abs().max())
    worst = float((outs["csr"] - outs["coo"]).abs().max())
    say("dim %d: max |csr - coo| = %.3g at max |coo| = %.3g" % (dim, worst, scale))
    us = {name: [] for name in outs}
    for _ in range(args.ab):
        for name in outs:
            us[name].append(run(name, args.steps))
    gb = (E * dim * 4 + N * dim * 4) / 1e9
    for name, v in us.items():
        med = statistics.median(v)
        say("dim %d %s: median %.0f us per call, min %.0f, max %.0f, spread %.0f; %.2f GB read + written = %.0f GB/s  (%s)"
            % (dim, name, med, min(v), max(v), max(v) - min(v), gb, gb / med * 1e6, " ".join("%.0f" % t for t in v)))
    diff = statistics.median(us["csr"]) - statistics.median(us["coo"])
    spread = max(us["coo"]) - min(us["coo"])
    say("dim %d: csr median - coo median = %.0f us, the coo baseline's own spread %.0f us: csr %s"
        % (dim, diff, spread, "NOT SLOWER beyond the spread" if diff <= spread else "SLOWER by more than the spread"))
    del h, outs
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
