#!/usr/bin/env python3
"""The feature gather of one papers100M-shaped batch (302 K rows of 128 features out of a table in HBM) with fp32 rows
against fp16 rows (`feat_store_dtype = f16`): fgnn_gather_rows alone, interleaved alternations of the two in one
process, median and spread of --ab rounds of --steps launches each, against the bytes each moves.
usage: feat_store_gather_ab.py [--rows 302000] [--dim 128] [--table-rows 20000000] [--ab 5] [--steps 200]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
from fgnn_hip import lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=302000)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--table-rows", type=int, default=20000000)
ap.add_argument("--ab", type=int, default=5)
ap.add_argument("--steps", type=int, default=200)
args = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
idx = torch.randint(0, args.table_rows, (args.rows,), device=dev, generator=g, dtype=torch.int32)
tables, outs = {}, {}
for name, dt in (("f32", torch.float32), ("f16", torch.float16)):
    tables[name] = torch.empty((args.table_rows, args.dim), dtype=dt, device=dev).normal_()
    outs[name] = torch.empty((args.rows, args.dim), dtype=dt, device=dev)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def run(name, n):
    e0.record()
    for _ in range(n):
        lib.gather_rows(outs[name], tables[name], src_index=idx)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


for name in tables:
    run(name, 20)
us = {name: [] for name in tables}
for _ in range(args.ab):
    for name in tables:
        us[name].append(run(name, args.steps))
for name, v in us.items():
    mb = args.rows * args.dim * tables[name].element_size() / 1e6
    med = statistics.median(v)
    print("%s rows: median %.1f us per gather, min %.1f, max %.1f, spread %.1f; %.1f MB read + %.1f MB written = "
          "%.0f GB/s  (%s)" % (name, med, min(v), max(v), max(v) - min(v), mb, mb, 2 * mb / med * 1e3,
                               " ".join("%.1f" % t for t in v)))
gain = statistics.median(us["f32"]) - statistics.median(us["f16"])
spread = max(max(v) - min(v) for v in us.values())
print("f32 median - f16 median = %.1f us, larger spread %.1f us: f16 %s"
      % (gain, spread, "FASTER" if gain > spread else "NOT FASTER beyond the spread"))
