#!/usr/bin/env python3
"""A/B of layer 0's keys and values in ONE library build, interleaved rounds in one process ("the fold"):

    python tools/ab_l0_fold.py [--config C3|C2] [--batch B] [--rounds R] [--reps N] [--json OUT]

  deep   : AFT_L0_FOLD=0 -- q, k, v of layer 0 by the model_dim-deep product over x0 (the arithmetic before the fold)
  folded : AFT_L0_FOLD=1 -- k, v from the row's input features on the tables the prologue launch builds in every call

Per arm: the mean forward time over the rounds and the round-to-round spread (max - min).  The gain counts when the means differ by more
than three times the larger spread (the bar of DESIGN.md 4.4b).  The spin-up is 4 000 forwards per arm (six seconds): with 300 the
clocks were still settling during the counted rounds and single rounds of an arm strayed by up to 13 us.  Also prints max|folded - deep| / |y|max: the two arms round differently."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from adafortitran_amd import _abi, _lib, synth  # noqa: E402
from adafortitran_amd.hip_ops import engine_from_numpy  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--spinup", type=int, default=4000)
ap.add_argument("--json", default="")
args = ap.parse_args()
c = {"C3": bench.C3, "C2": bench.C2}[args.config]
B = args.batch or c["batch"]
spec = bench._spec(c)
sd = synth.make_state_dict(**spec, adaptive_hidden=c["hidden"], max_seq_len=c["max_seq_len"], seed=bench.SEED)
inp = synth.make_inputs(B, ofdm=c["ofdm"], pilot=c["pilot"], seed=bench.SEED)
dev = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
pil = dev(inp["pilots"])
meta = [dev(inp[k]) for k in ("snr", "ds", "dop")] if c["hidden"] else [None] * 3
cfg = _abi.make_config(**spec, adaptive_hidden=c["hidden"])
eng = engine_from_numpy(cfg, sd, "cuda:0")
arms = {"deep": "0", "folded": "1"}
out = {n: torch.empty((B, *c["ofdm"]), dtype=torch.complex64, device="cuda:0") for n in arms}
for n, v in arms.items():
    _lib.set_switch("AFT_L0_FOLD", v)
    eng.forward(pil, *meta, out=out[n])
torch.cuda.synchronize()
diff = float((out["folded"] - out["deep"]).abs().max() / out["deep"].abs().max())


def timed(n, reps):
    _lib.set_switch("AFT_L0_FOLD", arms[n])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.forward(pil, *meta, out=out[n])
    e0.record()
    for _ in range(reps):
        eng.forward(pil, *meta, out=out[n])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for n in arms:                       # spin-up: clocks and caches settle before the first counted round
    timed(n, args.spinup)
times = {n: [] for n in arms}
for rnd in range(args.rounds):
    order = list(arms)
    for n in order[rnd % 2:] + order[:rnd % 2]:
        times[n].append(timed(n, args.reps))
_lib.set_switch("AFT_L0_FOLD", None)
mean = {n: statistics.mean(times[n]) for n in arms}
spread = {n: max(times[n]) - min(times[n]) for n in arms}
gain = mean["deep"] - mean["folded"]
bar = 3 * max(spread.values())
print(f"config {args.config} B={B}; forward us over {args.rounds} interleaved rounds of {args.reps}")
for n in arms:
    print(f"  {n:<7} mean {mean[n]:8.2f}  min {min(times[n]):8.2f}  max {max(times[n]):8.2f}  spread {spread[n]:6.2f}   rounds: " +
          " ".join(f"{t:.1f}" for t in times[n]))
print(f"  deep - folded = {gain:.2f} us ({100 * gain / mean['deep']:.2f} %); bar (3 x larger spread) = {bar:.2f} us: {'CLEARED' if gain > bar else 'not cleared'}")
print(f"max|folded - deep| / |y|max = {diff:.3e}")
if args.json:
    with open(args.json, "w") as fh:
        json.dump({"config": args.config, "batch": B, "rounds": args.rounds, "reps": args.reps, "max_rel_difference_of_outputs": float(f"{diff:.4e}"),
                   "arms": {n: {"mean_us": round(mean[n], 2), "spread_us": round(spread[n], 2), "rounds_us": [round(t, 2) for t in times[n]]}
                            for n in arms},
                   "gain_us": round(gain, 2), "bar_us": round(bar, 2), "cleared": bool(gain > bar)}, fh, indent=1)
        fh.write("\n")
