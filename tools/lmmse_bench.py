#!/usr/bin/env python3
"""What the LMMSE baseline (lmmse.LmmseEstimator, aft_lmmse_f32) costs on one MI355X, and what it measures.

    python tools/lmmse_bench.py [--out profiles/lmmse.json] [--sections k,h,e] [--frames 2048]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the kernel at 128 default-grid frames as device-event time over many back-to-back launches, in alternating rounds with the channel
      simulator (aft_channel_sim_f32) at the same batch: the two write the same [128, 120, 14] planes;
  p   for the profiler (``rocprofv3 --kernel-trace --stats -- python tools/lmmse_bench.py --child p``): 300 launches of each;
  h   host time per ``LmmseEstimator.forward`` call at 128 frames -- device-resident pilots with host meta (what SynthLoader and
      ResidentLoader yield) and all-CPU inputs (through the pinned ring) -- nothing else queued;
  e   the evaluation sweep (evaluation.get_test_stats) over make_pack sets, one per SNR at a mid delay spread and Doppler: LS (the
      pack's h_ls_full) vs LMMSE on the device vs lmmse_predicted_mse, in dB.  Reported, not asserted."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 240, "p": 240, "h": 240, "e": 420}     # seconds per child
BATCH = 128


def _stats(values, unit):
    return {f"median_{unit}": round(statistics.median(values), 4), f"min_{unit}": round(min(values), 4), f"max_{unit}": round(max(values), 4),
            f"spread_{unit}": round(max(values) - min(values), 4)}


def _kernels():
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LmmsePlan
    cfg = ChannelSimConfig()
    sim, plan = ChannelSimPlan(cfg, "cuda"), LmmsePlan(cfg, "cuda")
    _, pilots, meta = sim(1, 0, 0, 1, 1 << 40, BATCH)
    conds = [meta[:, k].contiguous() for k in range(3)]
    torch.cuda.synchronize()
    return {"lmmse": lambda: plan(pilots, *conds), "channel_sim": lambda: sim(1, 0, 0, 1, 1 << 40, BATCH)}


def section_k(a):
    import torch
    from train_loader_bench import _event_us
    variants = _kernels()
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(7):
        for k, fn in variants.items():
            us[k].append(_event_us(fn, 500))
    out = {k: _stats(v, "us") for k, v in us.items()}
    out["batch"] = BATCH
    out["note"] = "device-event time per call over 500 back-to-back calls: launch-rate bound for kernels this short; the kernel's own time is the profiler's"
    return out


def section_p(a):
    import torch
    for fn in _kernels().values():
        for _ in range(300):
            fn()
        torch.cuda.synchronize()
    return {"launches": 600}


def section_h(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader
    from adafortitran_amd.lmmse import LmmseEstimator
    cfg = ChannelSimConfig()
    model = LmmseEstimator(cfg).to("cuda")
    pilots, _, meta = next(iter(SynthLoader(cfg, BATCH, BATCH, device="cuda", seed=1)))
    inputs = {"device_pilots_host_meta": (pilots, meta), "cpu_pilots_host_meta": (pilots.cpu(), meta)}
    out = {}
    for name, (p, m) in inputs.items():
        for _ in range(20):
            model(p, m)
        torch.cuda.synchronize()
        per = []
        for _ in range(7):
            t0 = time.perf_counter()
            for _ in range(200):
                model(p, m)
            per.append((time.perf_counter() - t0) / 200 * 1e6)
            torch.cuda.synchronize()
        out[name] = _stats(per, "host_us_per_call")
    out["batch"] = BATCH
    return out


def section_e(a):
    import numpy as np
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.evaluation import get_test_stats
    from adafortitran_amd.lmmse import LmmseEstimator, lmmse_predicted_mse
    cfg = ChannelSimConfig()
    model = LmmseEstimator(cfg).to("cuda")
    ds, dop = 200.0, 800.0
    packs = {int(snr): make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop) for snr in cfg.snr_db}
    loaders = [(f"SNR_{snr}", ingest.ResidentLoader(p, cfg.pilot, BATCH, device="cuda", shuffle=False)) for snr, p in packs.items()]
    stats = get_test_stats(model, loaders)
    rows = []
    for snr, p in packs.items():
        ls = float((np.abs(p["h_ls_full"].astype(np.complex128) - p["h_ideal"]) ** 2).mean())
        rows.append({"snr_db": snr, "ls_db": round(10 * np.log10(ls), 3), "lmmse_db": round(stats[snr], 3),
                     "predicted_db": round(10 * np.log10(lmmse_predicted_mse(model.tables, snr, ds, dop)), 3)})
    return {"frames_per_set": a.frames, "delay_spread_ns": ds, "doppler_hz": dop, "rows": rows}


SECTIONS = {"k": section_k, "p": section_p, "h": section_h, "e": section_e}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmmse.json"))
    ap.add_argument("--sections", default="k,h,e")
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("lmmse_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/lmmse_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"lmmse_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
            record["stopped_at"], status = name, res.returncode
            break
        record[name] = json.loads(res.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps(record))
    return status


if __name__ == "__main__":
    sys.exit(main())
