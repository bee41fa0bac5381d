#!/usr/bin/env python3
"""What the coded link evaluation (linksim, aft_link_decode_f32) costs on one MI355X, and what it measures.

    python tools/link_coded_bench.py [--out profiles/link_coded.json] [--sections k,b] [--frames 256]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the Viterbi kernel at 128 default-grid frames per modulation order, rate and block length, as device-event time over many
      back-to-back launches, in alternating rounds with the soft kernel (aft_link_soft_f32 at one factor, with its LLR output) on the
      SAME tensors: the decoder reads exactly the tensor the soft kernel wrote.  Beside each figure: the blocks and trellis steps per
      call, the waves per workgroup and the time per trellis step of a wave (the serial chain's length);
  b   block-error rate, information-bit error rate and throughput (information bits of correct blocks per data element) over the
      simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames: perfect channel knowledge, the
      LMMSE estimate (on the device) and the interpolated LS estimate (the pack's h_ls_full).  Reported, not asserted."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 300, "b": 540}               # seconds per child
BATCH = 128
# (bits per symbol, rate, information bits per block)
KERNEL_CASES = ((2, "1/2", 512), (4, "1/2", 512), (4, "3/4", 512), (4, "1/2", 1024), (6, "2/3", 1024), (8, "3/4", 1024), (8, "1/2", 4090))
LINK_CASES = ((2, "1/2", 512), (4, "1/2", 512), (4, "3/4", 512), (6, "3/4", 512))


def _stats(values, unit):
    return {f"median_{unit}": round(statistics.median(values), 4), f"min_{unit}": round(min(values), 4), f"max_{unit}": round(max(values), 4),
            f"spread_{unit}": round(max(values) - min(values), 4)}


def section_k(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LinkDecodePlan, LinkSoftPlan, LmmsePlan
    from adafortitran_amd.linksim import CodeConfig, LinkConfig, frame_keys_torch
    from train_loader_bench import _event_us
    cfg = ChannelSimConfig()
    ideal, pilots, meta = ChannelSimPlan(cfg, "cuda")(1, 0, 0, 1, 1 << 40, BATCH)
    est = LmmsePlan(cfg, "cuda")(pilots, *(meta[:, k].contiguous() for k in range(3)))
    keys = frame_keys_torch(1, torch.arange(BATCH, device="cuda"))
    snr = meta[:, 0].double()
    sigma, scale = torch.pow(10.0, -snr / 20.0).float(), (1.0 / torch.pow(10.0, -snr / 10.0)).float()
    one = torch.ones(1, device="cuda")
    variants, shape = {}, {}
    for m in sorted({c[0] for c in KERNEL_CASES}):
        soft = LinkSoftPlan(LinkConfig(cfg, m), "cuda")
        llr = soft(ideal, est, keys, sigma, scale, one, want_llr=True)[1]
        variants[f"soft_m{m}_llr"] = lambda p=soft: p(ideal, est, keys, sigma, scale, one, want_llr=True)
        for mm, rate, K in KERNEL_CASES:
            if mm != m:
                continue
            code = CodeConfig(LinkConfig(cfg, m), K, rate)
            name = f"decode_m{m}_r{rate.replace('/', '')}_k{K}"
            variants[name] = lambda p=LinkDecodePlan(code, "cuda"), t=llr: p(t, keys)
            waves = min(16, code.blocks, max(1, (159 * 1024) // (8 * code.steps)))     # csrc/k_linkcode.hip link_code_waves
            shape[name] = {"blocks_per_frame": code.blocks, "steps": code.steps, "waves_per_workgroup": waves,
                           "rounds_per_wave": -(-code.blocks // waves), "soft": f"soft_m{m}_llr"}
    torch.cuda.synchronize()
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(5):
        for k, fn in variants.items():
            us[k].append(_event_us(fn, 100))
    out = {k: _stats(v, "us") for k, v in us.items()}
    for name, s in shape.items():
        chain = s["rounds_per_wave"] * s["steps"]
        out[name].update(s, ns_per_step_of_a_wave=round(out[name]["median_us"] * 1e3 / chain, 2),
                         soft_median_us=out[s["soft"]]["median_us"], soft_spread_us=out[s["soft"]]["spread_us"])
    out["batch"] = BATCH
    out["note"] = ("device-event time per call over 100 back-to-back calls, 5 alternating rounds: the allocations of the outputs and the "
                   "launch are inside it; the soft kernel runs at one factor with its LLR output, the decoder on that tensor")
    return out


def section_b(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import BlockErrorAccumulator, CodeConfig, LinkConfig
    from adafortitran_amd.lmmse import LmmseEstimator
    cfg = ChannelSimConfig()
    model = LmmseEstimator(cfg).to("cuda")
    ds, dop = 200.0, 800.0
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    codes = {c: CodeConfig(LinkConfig(cfg, c[0]), c[2], c[1]) for c in LINK_CASES}
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, ls = torch.from_numpy(pack["h_ideal"]).cuda(), torch.from_numpy(pack["h_ls_full"]).cuda()
        pilots = torch.from_numpy(np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]])).cuda()
        meta = torch.from_numpy(pack["meta"])
        accs = {(c, which): BlockErrorAccumulator(code, "cuda", seed=1) for c, code in codes.items() for which in ("perfect", "lmmse", "ls")}
        for lo in range(0, a.frames, BATCH):
            sl = slice(lo, lo + BATCH)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (c, which), acc in accs.items():
                acc.update(est[which], ideal[sl], cols)
        row = {"snr_db": int(snr)}
        for ((m, rate, K), which), acc in accs.items():
            row[f"m{m}_r{rate.replace('/', '')}_k{K}_{which}"] = {"bler": round(acc.result(), 4), "ber": round(acc.result_ber(), 6),
                                                                 "throughput": round(acc.result_throughput(), 4)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"frames_per_set": a.frames, "delay_spread_ns": ds, "doppler_hz": dop,
            "blocks_per_frame": {f"m{m}_r{rate.replace('/', '')}_k{K}": code.blocks for (m, rate, K), code in codes.items()}, "rows": rows}


SECTIONS = {"k": section_k, "b": section_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_coded.json"))
    ap.add_argument("--sections", default="k,b")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("link_coded_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_coded_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_coded_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
