#!/usr/bin/env python3
"""The GAT attention kernel of exact layer-wise inference (fgnn_csr_gat_attention: one wave per CSR row, edge weights
staged in LDS, no atomics, no E x H scratch, out overwritten) against the training-side attention on the identical edge
set expanded to COO (fgnn_gat_forward plus the zero fill of its output: a destination id per edge, E x H scores and
alphas, float atomics), over ALL rows of an R-MAT graph from the bench's generator (fgnn_hip.rmat, seed 42) at the bench
graph's average degree, for 8 heads of 32 and of 64 features.  Interleaved alternations of the two in one process, median
and spread of --ab rounds of --steps launches each; bytes counted as E x (feat row + el row + index) read and rows x H F
x 4 written -- what the CSR kernel needs, not what the baseline moves on top.  The outputs of the two are compared
first.  No ratio is fixed in advance: the verdict is printed as it comes out.
usage: csr_gat_ab.py [--num-node 4000000] [--num-edge 58000000] [--shapes 8x32 8x64] [--ab 7] [--steps 10]
                     [--out profiles/r12_a_csr_gat_ab.txt]"""
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
ap.add_argument("--shapes", nargs="+", default=["8x32", "8x64"], help="heads x features")
ap.add_argument("--ab", type=int, default=7)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_a_csr_gat_ab.txt"))
args = ap.parse_args()
lib.load()
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


indptr, indices, E = rmat.rmat_csr(args.num_node, args.num_edge, seed=42, device=dev)
N, E = args.num_node, indices.numel()
deg = (indptr[1:].long() & 0xFFFFFFFF) - (indptr[:-1].long() & 0xFFFFFFFF)
col = torch.repeat_interleave(torch.arange(N, device=dev, dtype=torch.int32), deg)  # the COO's destination per edge
split = nn.csr_split_length()
say("R-MAT (fgnn_hip.rmat, seed 42): %d nodes, %d edges; longest row %d, %d rows above the split length %d, %d rows "
    "without an edge" % (N, E, int(deg.max()), int((deg > split).sum()), split, int((deg == 0).sum())))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for shape in args.shapes:
    H, F = (int(v) for v in shape.split("x"))
    feat = torch.empty((N, H, F), dtype=torch.float32, device=dev).normal_()
    el, er = (torch.empty((N, H), dtype=torch.float32, device=dev).normal_() for _ in range(2))
    outs = {"csr": torch.empty((N, H, F), dtype=torch.float32, device=dev),
            "coo": torch.empty((N, H, F), dtype=torch.float32, device=dev)}
    alpha = torch.empty((E, H), dtype=torch.float32, device=dev)
    say("%s: the COO baseline writes and reads %.0f MB of alphas, %.0f MB of scratch and reads %.0f MB of destination "
        "ids on top; the CSR kernel's workspace is %.1f MB"
        % (shape, 4 * E * H / 1e6, lib.load().fgnn_gat_workspace_bytes(E, N, H) / 1e6, 4 * E / 1e6,
           lib.load().fgnn_csr_gat_workspace_bytes(N, E, H, F) / 1e6))

    def launch(name):
        if name == "csr":
            nn.csr_gat_attention_into(outs["csr"], feat, el, er, indptr, indices)
        else:
            outs["coo"].zero_()
            nn.gat_forward_into(outs["coo"], alpha, feat, el, er, indices, col)

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
    say("%s: max |csr - coo| = %.3g at max |coo| = %.3g" % (shape, worst, scale))
    us = {name: [] for name in outs}
    for _ in range(args.ab):
        for name in outs:
            us[name].append(run(name, args.steps))
    gb = (E * (H * F * 4 + H * 4 + 4) + N * H * F * 4) / 1e9
    for name, v in us.items():
        med = statistics.median(v)
        say("%s %s: median %.0f us per call, min %.0f, max %.0f, spread %.0f; %.2f GB read + written = %.0f GB/s  (%s)"
            % (shape, name, med, min(v), max(v), max(v) - min(v), gb, gb / med * 1e6, " ".join("%.0f" % t for t in v)))
    med = {name: statistics.median(v) for name, v in us.items()}
    spread = max(max(v) - min(v) for v in us.values())
    diff = med["csr"] - med["coo"]
    verdict = ("NO DIFFERENCE beyond the spread" if abs(diff) <= spread else
               "csr SLOWER by more than the spread" if diff > 0 else "csr FASTER by more than the spread")
    say("%s: csr median / coo median = %.2f (csr - coo = %.0f us, the larger spread of the two %.0f us): %s"
        % (shape, med["csr"] / med["coo"], diff, spread, verdict))
    del feat, el, er, outs, alpha
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
