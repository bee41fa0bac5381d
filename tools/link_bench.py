#!/usr/bin/env python3
"""What the link-level error count (linksim, aft_link_errors_f32) costs on one MI355X, and what it measures.

    python tools/link_bench.py [--out profiles/link.json] [--sections k,e] [--frames 1024]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the kernel at 128 default-grid frames for each modulation order as device-event time over many back-to-back launches, in
      alternating rounds with the LS-baseline metric (aft_ls_mse_db_f32) on the SAME two tensors: it reads the same bytes (two
      complex64 [128, 120, 14] arrays, 3.44 MB) and does next to no arithmetic, which makes it the yardstick;
  p   for the profiler (``rocprofv3 --kernel-trace --stats -- python tools/link_bench.py --child p``): 300 launches of each; the
      kernel's own time is the profiler's, and bytes over that time the achieved bandwidth (``--stats-csv`` turns the profiler's
      kernel_stats.csv into that table);
  e   bit-error rates over the simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames: perfect
      channel knowledge, the LMMSE estimate (on the device) and the interpolated LS estimate (the pack's h_ls_full), per modulation
      order.  Reported, not asserted."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 240, "p": 240, "e": 420}     # seconds per child
BATCH = 128
ORDERS = (2, 4, 6, 8)
BYTES = 2 * BATCH * 120 * 14 * 8             # what either kernel reads: ideal and est


def _stats(values, unit):
    return {f"median_{unit}": round(statistics.median(values), 4), f"min_{unit}": round(min(values), 4), f"max_{unit}": round(max(values), 4),
            f"spread_{unit}": round(max(values) - min(values), 4)}


def _kernels():
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LinkPlan, LmmsePlan, ls_mse_db
    from adafortitran_amd.linksim import LinkConfig, frame_keys_torch
    cfg = ChannelSimConfig()
    ideal, pilots, meta = ChannelSimPlan(cfg, "cuda")(1, 0, 0, 1, 1 << 40, BATCH)
    est = LmmsePlan(cfg, "cuda")(pilots, *(meta[:, k].contiguous() for k in range(3)))
    keys = frame_keys_torch(1, torch.arange(BATCH, device="cuda"))
    sigma = torch.pow(10.0, -meta[:, 0].double() / 20.0).float()
    plans = {m: LinkPlan(LinkConfig(cfg, m), "cuda") for m in ORDERS}
    torch.cuda.synchronize()
    variants = {f"link_m{m}": (lambda p=p: p(ideal, est, keys, sigma)) for m, p in plans.items()}
    variants["ls_mse_db"] = lambda: ls_mse_db(est, ideal)
    return variants


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
    out["batch"], out["bytes_read"] = BATCH, BYTES
    out["note"] = "device-event time per call over 500 back-to-back calls: launch-rate bound for kernels this short; the kernel's own time is the profiler's"
    return out


def section_p(a):
    import torch
    for fn in _kernels().values():
        for _ in range(300):
            fn()
        torch.cuda.synchronize()
    return {"launches": 300 * (len(ORDERS) + 1)}


def section_e(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import LinkAccumulator, LinkConfig
    from adafortitran_amd.lmmse import LmmseEstimator
    cfg = ChannelSimConfig()
    model = LmmseEstimator(cfg).to("cuda")
    ds, dop = 200.0, 800.0
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, ls = torch.from_numpy(pack["h_ideal"]).cuda(), torch.from_numpy(pack["h_ls_full"]).cuda()
        pilots = torch.from_numpy(np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]])).cuda()
        meta = torch.from_numpy(pack["meta"])
        accs = {(m, which): LinkAccumulator(LinkConfig(cfg, m), "cuda", seed=1) for m in ORDERS for which in ("perfect", "lmmse", "ls")}
        for lo in range(0, a.frames, BATCH):
            sl = slice(lo, lo + BATCH)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (m, which), acc in accs.items():
                acc.update(est[which], ideal[sl], cols)
        row = {"snr_db": int(snr)}
        for (m, which), acc in accs.items():
            row[f"m{m}_{which}"] = float(f"{acc.result():.4e}")
        rows.append(row)
    return {"frames_per_set": a.frames, "delay_spread_ns": ds, "doppler_hz": dop, "rows": rows}


SECTIONS = {"k": section_k, "p": section_p, "e": section_e}


def stats_table(path):
    """The profiler's kernel_stats.csv -> {kernel: {calls, mean_us, GB_per_s}} for the kernels of section p."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if "link_errors_kernel" in name or "ls_mse_db_kernel" in name:
                mean_ns = float(row["AverageNs"])
                out[name] = {"calls": int(row["Calls"]), "mean_us": round(mean_ns / 1e3, 3), "GB_per_s": round(BYTES / mean_ns, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link.json"))
    ap.add_argument("--sections", default="k,e")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--child", default="")
    ap.add_argument("--stats-csv", default="")
    a = ap.parse_args()
    if a.stats_csv:
        print(json.dumps(stats_table(a.stats_csv), indent=1))
        return 0
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("link_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
