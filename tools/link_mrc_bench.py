#!/usr/bin/env python3
"""What receive diversity on the link (linksim "the diversity link", aft_link_mrc_f32) costs on one MI355X, and what it measures.

    python tools/link_mrc_bench.py [--out profiles/link_mrc.json] [--sections k,b] [--frames 256]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the combiner kernel at 128 groups of the default grid with R = 1, 2, 4 branches, per modulation order, at one factor with
      its LLR output, as device-event time over many back-to-back launches, in alternating rounds with the soft kernel
      (aft_link_soft_f32, one factor, with its LLR output) on the SAME 128 R frames.  The same tree and the same process: a
      description, not a target;
  b   bit-error rate, achievable rate (GMI, the best of the default factor grid) and LDPC block-error rate (rate 1/2) at 16-QAM
      over the simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames, with R = 1, 2, 4
      branches: perfect channel knowledge, the LMMSE estimate (on the device) and the interpolated LS estimate.  Every R sees
      the same frames, so R branches leave ``frames / R`` transmissions.  Reported, not asserted."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 240, "b": 540}     # seconds per child
GROUPS = 128
BRANCHES = (1, 2, 4)
BITS = 4                          # section b: 16-QAM


def _stats(values, unit):
    return {f"median_{unit}": round(statistics.median(values), 4), f"min_{unit}": round(min(values), 4), f"max_{unit}": round(max(values), 4),
            f"spread_{unit}": round(max(values) - min(values), 4)}


def _tensors(frames):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LmmsePlan
    from adafortitran_amd.linksim import frame_keys_torch
    cfg = ChannelSimConfig()
    ideal, pilots, meta = ChannelSimPlan(cfg, "cuda")(1, 0, 0, 1, 1 << 40, frames)
    est = LmmsePlan(cfg, "cuda")(pilots, *(meta[:, k].contiguous() for k in range(3)))
    keys = frame_keys_torch(1, torch.arange(frames, device="cuda"))
    snr = meta[:, 0].double()
    sigma, scale = torch.pow(10.0, -snr / 20.0).float(), (1.0 / torch.pow(10.0, -snr / 10.0)).float()
    return cfg, ideal, est, keys, sigma, scale


def _measure(variants):
    import torch
    from train_loader_bench import _event_us
    torch.cuda.synchronize()
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(5):
        for k, fn in variants.items():
            us[k].append(_event_us(fn, 100))
    return {k: _stats(v, "us") for k, v in us.items()}


NOTE = ("device-event time per call over 100 back-to-back calls, 5 alternating rounds: the allocations of the outputs and the launch are "
        "inside it; both kernels run at one factor with their LLR output on the same frames (LMMSE estimates, the simulator's conditions "
        "drawn per frame, so the weights are mixed); the combiner writes 128 groups of LLRs, the soft kernel 128 R frames of them")


def section_k(a):
    import torch
    from adafortitran_amd.hip_ops import LinkMrcPlan, LinkSoftPlan
    from adafortitran_amd.linksim import BITS_PER_SYMBOL, LinkConfig
    one = torch.ones(1, device="cuda")
    variants = {}
    for R in BRANCHES:
        cfg, ideal, est, keys, sigma, scale = _tensors(GROUPS * R)
        s = scale.view(GROUPS, R).double()
        rho, lead = (s / s[:, :1]).float().reshape(-1), scale[::R].contiguous()
        for m in BITS_PER_SYMBOL:
            link = LinkConfig(cfg, m)
            variants[f"mrc_m{m}_r{R}"] = lambda p=LinkMrcPlan(link, "cuda", R), t=(ideal, est, keys, sigma, rho, lead): p(*t, one, want_llr=True)
            variants[f"soft_m{m}_frames{GROUPS * R}"] = lambda p=LinkSoftPlan(link, "cuda"), t=(ideal, est, keys, sigma, scale): p(*t, one, want_llr=True)
    out = _measure(variants)
    for R in BRANCHES:
        for m in BITS_PER_SYMBOL:
            row = out[f"mrc_m{m}_r{R}"]
            row["soft_same_frames_median_us"] = out[f"soft_m{m}_frames{GROUPS * R}"]["median_us"]
            row["ns_per_branch_element"] = round(row["median_us"] * 1e3 / (GROUPS * R * 1680), 4)
    out["groups"], out["note"] = GROUPS, NOTE
    return out


def section_b(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import DEFAULT_FACTORS, LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator
    from adafortitran_amd.lmmse import LmmseEstimator
    cfg = ChannelSimConfig()
    link = LinkConfig(cfg, BITS)
    code = LdpcConfig(link, "1/2")
    model = LmmseEstimator(cfg).to("cuda")
    ds, dop = 200.0, 800.0
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    batch = 128
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, ls = torch.from_numpy(pack["h_ideal"]).cuda(), torch.from_numpy(pack["h_ls_full"]).cuda()
        pilots = torch.from_numpy(np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]])).cuda()
        meta = torch.from_numpy(pack["meta"])
        accs = {(R, which): (LinkAccumulator(link, "cuda", seed=1, branches=R),
                             RateAccumulator(link, "cuda", seed=1, factors=DEFAULT_FACTORS, branches=R),
                             LdpcBlockErrorAccumulator(code, "cuda", seed=1, branches=R))
                for R in BRANCHES for which in ("perfect", "lmmse", "ls")}
        for lo in range(0, a.frames, batch):
            sl = slice(lo, lo + batch)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (R, which), three in accs.items():
                for acc in three:
                    acc.update(est[which], ideal[sl], cols)
        row = {"snr_db": int(snr)}
        for (R, which), (hard, rate, bler) in accs.items():
            row[f"r{R}_{which}"] = {"ber": round(hard.result(), 6), "gmi": round(rate.result_gmi(), 4), "ldpc_bler": round(bler.result(), 4),
                                    "ldpc_iterations": round(bler.result_iterations(), 3)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"frames_per_set": a.frames, "bits_per_symbol": BITS, "ldpc": "rate 1/2, n = 1536", "blocks_per_transmission": code.blocks,
            "delay_spread_ns": ds, "doppler_hz": dop, "rows": rows}


SECTIONS = {"k": section_k, "b": section_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_mrc.json"))
    ap.add_argument("--sections", default="k,b")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.frames < 1 or a.frames % (128 if a.frames > 128 else max(BRANCHES)):
        ap.error("--frames: a multiple of 4 up to 128, or a multiple of 128")
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("link_mrc_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_mrc_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_mrc_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
