#!/usr/bin/env python3
"""What the soft link evaluation (linksim, aft_link_soft_f32) costs on one MI355X, and what it measures.

    python tools/link_soft_bench.py [--out profiles/link_soft.json] [--sections k,r] [--frames 512]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the kernel at 128 default-grid frames and the eight default factors, for each modulation order with and without the LLR output,
      as device-event time over many back-to-back launches, in alternating rounds with the hard kernel (aft_link_errors_f32) at the
      same order on the SAME tensors; the hard kernel's own spread over the rounds of that run is reported beside every figure, and
      the bytes the call moves over its time as GB/s against the 6.29 TB/s copy ceiling;
  p   for the profiler (``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/link_soft_bench.py --child p``): 300
      launches of each; the kernel's own time is the profiler's (``--stats-csv FILE`` turns the profiler's kernel_stats.csv into a
      table and adds it to the record at ``--out`` as section ``p``);
  r   achievable rates in bit/symbol over the simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames``
      frames: perfect channel knowledge, the LMMSE estimate (on the device) and the interpolated LS estimate (the pack's h_ls_full),
      per modulation order at each of ``linksim.DEFAULT_FACTORS`` and their best.  Reported, not asserted."""
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

LIMITS = {"k": 300, "p": 300, "r": 540}     # seconds per child
BATCH = 128
ORDERS = (2, 4, 6, 8)
ELEMENTS = 120 * 14
COPY_CEILING_GB_S = 6290.0                   # the copy ceiling the project quotes


def bytes_moved(m, with_llr):
    """(read, written) per call: ideal and est in, the losses and (with the LLR output) m float32 per element out."""
    return 2 * BATCH * ELEMENTS * 8, BATCH * 8 * 4 + (BATCH * ELEMENTS * m * 4 if with_llr else 0)


def _stats(values, unit):
    return {f"median_{unit}": round(statistics.median(values), 4), f"min_{unit}": round(min(values), 4), f"max_{unit}": round(max(values), 4),
            f"spread_{unit}": round(max(values) - min(values), 4)}


def _kernels():
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LinkPlan, LinkSoftPlan, LmmsePlan
    from adafortitran_amd.linksim import DEFAULT_FACTORS, LinkConfig, frame_keys_torch
    cfg = ChannelSimConfig()
    ideal, pilots, meta = ChannelSimPlan(cfg, "cuda")(1, 0, 0, 1, 1 << 40, BATCH)
    est = LmmsePlan(cfg, "cuda")(pilots, *(meta[:, k].contiguous() for k in range(3)))
    keys = frame_keys_torch(1, torch.arange(BATCH, device="cuda"))
    snr = meta[:, 0].double()
    sigma, scale = torch.pow(10.0, -snr / 20.0).float(), (1.0 / torch.pow(10.0, -snr / 10.0)).float()
    factors = torch.tensor(DEFAULT_FACTORS, dtype=torch.float32, device="cuda")
    variants = {}
    for m in ORDERS:
        hard, soft = LinkPlan(LinkConfig(cfg, m), "cuda"), LinkSoftPlan(LinkConfig(cfg, m), "cuda")
        variants[f"hard_m{m}"] = lambda p=hard: p(ideal, est, keys, sigma)
        variants[f"soft_m{m}"] = lambda p=soft: p(ideal, est, keys, sigma, scale, factors)
        variants[f"soft_m{m}_llr"] = lambda p=soft: p(ideal, est, keys, sigma, scale, factors, want_llr=True)
    torch.cuda.synchronize()
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
            us[k].append(_event_us(fn, 300))
    out = {k: _stats(v, "us") for k, v in us.items()}
    for m in ORDERS:
        for name, with_llr in ((f"soft_m{m}", False), (f"soft_m{m}_llr", True)):
            read, written = bytes_moved(m, with_llr)
            gb_s = (read + written) / (out[name]["median_us"] * 1e3)
            out[name].update(bytes_read=read, bytes_written=written, GB_per_s=round(gb_s, 1),
                             share_of_copy_ceiling=round(gb_s / COPY_CEILING_GB_S, 4), hard_spread_us=out[f"hard_m{m}"]["spread_us"])
    out["batch"], out["factors"] = BATCH, 8
    out["note"] = ("device-event time per call over 300 back-to-back calls, 7 alternating rounds: the allocations of the outputs and the "
                   "launch are inside it, so a kernel shorter than a launch shows the launch rate; the kernel's own time is the profiler's")
    return out


def section_p(a):
    import torch
    for fn in _kernels().values():
        for _ in range(300):
            fn()
        torch.cuda.synchronize()
    return {"launches": 300 * 3 * len(ORDERS)}


def section_r(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import DEFAULT_FACTORS, LinkConfig, RateAccumulator
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
        accs = {(m, which): RateAccumulator(LinkConfig(cfg, m), "cuda", seed=1, factors=DEFAULT_FACTORS)
                for m in ORDERS for which in ("perfect", "lmmse", "ls")}
        for lo in range(0, a.frames, BATCH):
            sl = slice(lo, lo + BATCH)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (m, which), acc in accs.items():
                acc.update(est[which], ideal[sl], cols)
        row = {"snr_db": int(snr)}
        for (m, which), acc in accs.items():
            rates = acc.result()
            row[f"m{m}_{which}"] = {"rates": [round(v, 4) for v in rates], "best": round(max(rates), 4),
                                    "best_factor": DEFAULT_FACTORS[int(np.argmax(rates))]}
        rows.append(row)
    return {"frames_per_set": a.frames, "delay_spread_ns": ds, "doppler_hz": dop, "factors": list(DEFAULT_FACTORS), "rows": rows}


SECTIONS = {"k": section_k, "p": section_p, "r": section_r}


def stats_table(path):
    """The profiler's kernel_stats.csv -> {kernel: {calls, mean_us}} for the kernels of section p (both LLR forms of an order share a
    kernel name: their mean is over both)."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if "link_soft_kernel" in name or "link_errors_kernel" in name:
                out[name] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 3),
                             "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_soft.json"))
    ap.add_argument("--sections", default="k,r")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--child", default="")
    ap.add_argument("--stats-csv", default=None)
    a = ap.parse_args()
    if a.stats_csv is not None:
        table = stats_table(a.stats_csv)
        if os.path.exists(a.out):
            with open(a.out) as fh:
                record = json.load(fh)
            record["p"] = table
            with open(a.out, "w") as fh:
                json.dump(record, fh, indent=1)
                fh.write("\n")
        print(json.dumps(table, indent=1))
        return 0
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("link_soft_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_soft_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_soft_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
