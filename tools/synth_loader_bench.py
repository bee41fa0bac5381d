#!/usr/bin/env python3
"""What the on-device channel simulator (chansim.SynthLoader, aft_channel_sim_f32) costs on one MI355X, and whether a model learns from it.

    python tools/synth_loader_bench.py [--out profiles/synth_loader.json] [--sections k,h,d,t] [--train-steps 300]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the kernel alone at 16 / 64 / 128 default-grid frames as device-event times over many launches, interleaved with the frame gather
      of ingest.ResidentLoader (tools/train_loader_bench.py's variant) at the same batch sizes;
  h   host time per ``next()`` of a SynthLoader epoch and of a ResidentLoader epoch at 128 frames, nothing else queued;
  d   the 128-frame training step of tools/train_bench.py's loop fed by a SynthLoader epoch and by a ResidentLoader epoch (the code path
      that existed before the simulator), in alternating rounds in one process: median and spread of both; the verdict holds the
      difference of the medians against the ResidentLoader-fed step's own max - min in this run, no threshold fixed in advance;
  t   a short training at a fixed seed fed by SynthLoader: the loss per window of steps next to the LS baseline (the pilots' linear
      interpolation, chansim.ls_interpolate's weights applied on the device) and the LMMSE baseline (lmmse.LmmseEstimator, matched to
      each frame's condition: the best linear estimator) of the SAME frames, all three as the trainer's MSELoss over the real view.
      Reported, not asserted."""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 240, "p": 240, "h": 240, "d": 420, "t": 420}     # seconds per child
FRAMES = 8192                                         # the resident pack the ResidentLoader side draws from


def _stats(values, unit):
    return {f"median_{unit}": round(statistics.median(values), 4), f"min_{unit}": round(min(values), 4), f"max_{unit}": round(max(values), 4),
            f"spread_{unit}": round(max(values) - min(values), 4)}


def section_k(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan
    from train_loader_bench import _event_us, _gather_variants
    plan = ChannelSimPlan(ChannelSimConfig(), "cuda")
    out = {}
    for batch in (16, 64, 128):
        variants = {"channel_sim": lambda: plan(1, 0, 0, 1, 1 << 40, batch),
                    "frame_gather_hbm": _gather_variants(FRAMES, batch, batch)["frame_gather_hbm"]}
        for fn in variants.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(7):
            for k, fn in variants.items():
                us[k].append(_event_us(fn, 500))
        out[str(batch)] = {k: _stats(v, "us") for k, v in us.items()}
    out["note"] = "device-event time per call over 500 back-to-back calls: launch-rate bound for kernels this short; the kernel's own time is the profiler's"
    return out


def section_p(a):
    """For the profiler (``rocprofv3 --kernel-trace --stats -- python tools/synth_loader_bench.py --child p``): 300 launches each of
    channel_sim_kernel and of frame_gather_kernel at 16, 64 and 128 frames (the trace tells them apart by name and grid size)."""
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan
    from train_loader_bench import _gather_variants
    plan = ChannelSimPlan(ChannelSimConfig(), "cuda")
    for batch in (16, 64, 128):
        gather = _gather_variants(FRAMES, batch, batch)["frame_gather_hbm"]
        for _ in range(300):
            plan(1, 0, 0, 1, 1 << 40, batch)
        torch.cuda.synchronize()
        for _ in range(300):
            gather()
        torch.cuda.synchronize()
    return {"launches": 1800}


def _loaders(batch):
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, make_pack
    cfg = ChannelSimConfig()
    pack = make_pack(cfg, FRAMES, seed=1)
    return (SynthLoader(cfg, batch, FRAMES, device="cuda", seed=2),
            ingest.ResidentLoader(pack, cfg.pilot, batch, device="cuda", seed=2))


def section_h(a):
    import torch
    out = {}
    for name, loader in zip(("synth_loader", "resident_loader"), _loaders(128)):
        for _ in loader:
            pass
        torch.cuda.synchronize()
        per = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in loader:
                pass
            per.append((time.perf_counter() - t0) / len(loader) * 1e6)
            torch.cuda.synchronize()
        out[name] = {**_stats(per, "host_us_per_next"), "batches_per_epoch": len(loader)}
    return out


def section_d(a):
    import torch
    from train_loader_bench import _trainer
    synth, resident = _loaders(128)
    step = _trainer(128)
    steps = min(len(synth), len(resident), 60)

    def fed(loader):
        def run():                                  # a new epoch per round
            for b in itertools.islice(loader, steps):
                step(*b)
        return run

    variants = {"resident_loader": fed(resident), "synth_loader": fed(synth)}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(7):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    res = {k: _stats(v, "ms") for k, v in ms.items()}
    res["steps_per_round"], res["rounds"] = steps, 7
    res["synth_minus_resident_ms"] = round(res["synth_loader"]["median_ms"] - res["resident_loader"]["median_ms"], 4)
    res["margin_ms_resident_spread"] = res["resident_loader"]["spread_ms"]
    res["not_slower_beyond_margin"] = bool(res["synth_minus_resident_ms"] <= res["margin_ms_resident_spread"])
    return res


def section_t(a):
    import numpy as np
    import torch
    import train_bench
    from adafortitran_amd import chansim
    from adafortitran_amd.lmmse import LmmseEstimator
    from adafortitran_amd.optim import ShardedFlatAdam
    cfg = chansim.ChannelSimConfig()
    wiener = LmmseEstimator(cfg).to("cuda")
    torch.manual_seed(0)
    model = train_bench.build("adafortitran", 0.0).train()
    opt = ShardedFlatAdam(model.parameters(), lr=a.lr)
    loader = chansim.SynthLoader(cfg, 128, 128 * a.train_steps, device="cuda", seed=7)
    # the LS baseline's interpolation weights, from ls_interpolate applied to unit pilots
    eye = np.eye(cfg.pilot[0] * cfg.pilot[1]).reshape(-1, *cfg.pilot)
    w = torch.from_numpy(chansim.ls_interpolate(cfg, eye).reshape(len(eye), -1)).cuda()          # [Ps*Pt, S*T]
    losses, ls, lm = [], [], []
    for pilots, ideal, meta in loader:
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(torch.view_as_real(model(pilots, meta)), torch.view_as_real(ideal))
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        base = (pilots.reshape(len(pilots), -1) @ w).reshape(ideal.shape)
        ls.append(torch.nn.functional.mse_loss(torch.view_as_real(base), torch.view_as_real(ideal)))
        with torch.no_grad():
            lm.append(torch.nn.functional.mse_loss(torch.view_as_real(wiener(pilots, meta)), torch.view_as_real(ideal)))
    losses, ls, lm = (torch.stack(v).cpu().numpy() for v in (losses, ls, lm))
    win = max(1, a.train_steps // 12)
    curve = [{"steps": [lo, min(lo + win, len(losses))], "loss": round(float(losses[lo:lo + win].mean()), 6),
              "ls_baseline": round(float(ls[lo:lo + win].mean()), 6), "lmmse_baseline": round(float(lm[lo:lo + win].mean()), 6)}
             for lo in range(0, len(losses), win)]
    return {"seed": 7, "batch": 128, "steps": int(len(losses)), "lr": a.lr, "dropout": 0.0, "finite": bool(np.isfinite(losses).all()),
            "curve": curve, "final_loss": curve[-1]["loss"], "final_ls_baseline": curve[-1]["ls_baseline"],
            "final_lmmse_baseline": curve[-1]["lmmse_baseline"], "beats_ls": bool(curve[-1]["loss"] < curve[-1]["ls_baseline"]),
            "beats_lmmse": bool(curve[-1]["loss"] < curve[-1]["lmmse_baseline"])}


SECTIONS = {"k": section_k, "p": section_p, "h": section_h, "d": section_d, "t": section_t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_loader.json"))
    ap.add_argument("--sections", default="k,h,d,t")
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("synth_loader_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/synth_loader_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--train-steps", str(a.train_steps), "--lr", str(a.lr)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"synth_loader_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
