#!/usr/bin/env python3
"""Per-kernel times of the training conv stack from a `rocprofv3 --kernel-trace --stats --output-format csv` run of
tools/long_grid_conv_time.py: the conv-stack launches of the forward and of the dgrad share one kernel, told apart by their
position -- a dgrad launch follows the weight-flip kernel.  Prints mean us per launch of forward, flip, dgrad and weight-gradient
kernels, and the head / tail launches of the inference engine.
Usage: python tools/conv_trace_split.py <rocprofv3 output directory>"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

paths = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True)
rows = []
for p in paths:
    with open(p) as fh:
        rows += list(csv.DictReader(fh))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
acc = defaultdict(list)
prev = ""
for r in rows:
    name = r["Kernel_Name"]
    us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    if "conv_flip_weights" in name:
        kind = "flip"
    elif "wgrad" in name or "chsum" in name:
        kind = "wgrad"
    elif ("conv_stack_kernel<true" in name or "conv_stream" in name and "true" in name) and "conv_flip_weights" in prev:
        kind = "dgrad"
    elif "conv_stack_kernel<true" in name or ("conv_stream" in name and "true" in name):
        kind = "train_fwd"
    elif "conv" in name:
        kind = "inference:" + name.split("(")[0].split("<")[0]
    else:
        kind = None
    if kind:
        acc[kind].append(us)
    prev = name
print(json.dumps({k: dict(launches=len(v), mean_us=round(sum(v) / len(v), 1)) for k, v in sorted(acc.items())}))
