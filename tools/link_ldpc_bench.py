#!/usr/bin/env python3
"""What the LDPC-coded link evaluation (linksim, aft_link_ldpc_f32) costs on one MI355X, and what it measures.

    python tools/link_ldpc_bench.py [--out profiles/link_ldpc.json] [--sections k,i,b] [--frames 256]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the layered min-sum kernel at 128 default-grid frames per modulation order and rate, as device-event time over many
      back-to-back launches, in alternating rounds with the Viterbi kernel (aft_link_decode_f32, the convolutional code at the same
      rate and the same information bits per block) and the soft kernel (aft_link_soft_f32 at one factor, with its LLR output) on
      the SAME tensors.  Beside each figure: the blocks per frame, the waves per workgroup, the edges of the base matrix, the mean
      iterations the blocks ran and the time per (iteration, edge) of a wave;
  i   the same kernel against max_iters on one tensor, with the mean iterations that were run;
  b   block-error rate, throughput (information bits of correct blocks per data element) and mean iterations over the simulator's
      SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames: perfect channel knowledge, the LMMSE
      estimate (on the device) and the interpolated LS estimate, for the LDPC code and for the convolutional code at the same rate.
      Reported, not asserted."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 300, "i": 240, "b": 540}     # seconds per child
BATCH = 128
# (bits per symbol, rate): n = 1536, K = 768 / 1024 / 1152
KERNEL_CASES = ((2, "1/2"), (4, "1/2"), (4, "3/4"), (6, "2/3"), (8, "3/4"), (8, (3, 4)), (4, (3, 32)))
ITERS = (1, 2, 5, 10, 20, 50)
LINK_CASES = ((2, "1/2"), (4, "1/2"), (4, "3/4"), (6, "3/4"))


def _stats(values, unit):
    return {f"median_{unit}": round(statistics.median(values), 4), f"min_{unit}": round(min(values), 4), f"max_{unit}": round(max(values), 4),
            f"spread_{unit}": round(max(values) - min(values), 4)}


def _name(rate):
    return rate.replace("/", "") if isinstance(rate, str) else f"{rate[0]}x{rate[1]}"


def _waves(code):
    per_wave = 2 * code.coded_bits + 64 * code.edges                             # csrc/k_linkldpc.hip link_ldpc_waves
    return min(16, code.blocks, max(1, (150 * 1024) // per_wave))


def _tensors():
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LmmsePlan
    from adafortitran_amd.linksim import frame_keys_torch
    cfg = ChannelSimConfig()
    ideal, pilots, meta = ChannelSimPlan(cfg, "cuda")(1, 0, 0, 1, 1 << 40, BATCH)
    est = LmmsePlan(cfg, "cuda")(pilots, *(meta[:, k].contiguous() for k in range(3)))
    keys = frame_keys_torch(1, torch.arange(BATCH, device="cuda"))
    snr = meta[:, 0].double()
    sigma, scale = torch.pow(10.0, -snr / 20.0).float(), (1.0 / torch.pow(10.0, -snr / 10.0)).float()
    return cfg, ideal, est, keys, sigma, scale, torch.ones(1, device="cuda")


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
        "inside it; the soft kernel runs at one factor with its LLR output, the decoders on that tensor (LMMSE estimates, the simulator's "
        "conditions drawn per frame)")


def section_k(a):
    from adafortitran_amd.hip_ops import LinkDecodePlan, LinkLdpcPlan, LinkSoftPlan
    from adafortitran_amd.linksim import CodeConfig, LdpcConfig, LinkConfig
    cfg, ideal, est, keys, sigma, scale, one = _tensors()
    variants, shape = {}, {}
    for m in sorted({c[0] for c in KERNEL_CASES}):
        link = LinkConfig(cfg, m)
        soft = LinkSoftPlan(link, "cuda")
        llr = soft(ideal, est, keys, sigma, scale, one, want_llr=True)[1]
        variants[f"soft_m{m}_llr"] = lambda p=soft: p(ideal, est, keys, sigma, scale, one, want_llr=True)
        for mm, rate in KERNEL_CASES:
            if mm != m:
                continue
            code = LdpcConfig(link, rate)
            plan = LinkLdpcPlan(code, "cuda")
            name = f"ldpc_m{m}_r{_name(rate)}"
            variants[name] = lambda p=plan, t=llr: p(t, keys)
            counts = plan(llr, keys)[0].sum(dim=0).tolist()
            waves = _waves(code)
            shape[name] = {"blocks_per_frame": code.blocks, "info_bits": code.info_bits, "edges": code.edges, "waves_per_workgroup": waves,
                           "rounds_per_wave": -(-code.blocks // waves), "mean_iterations": round(counts[2] / (BATCH * code.blocks), 3),
                           "bler": round(counts[1] / (BATCH * code.blocks), 4), "soft": f"soft_m{m}_llr"}
            if isinstance(rate, str):
                conv = CodeConfig(link, code.info_bits, rate)
                variants[f"viterbi_m{m}_r{_name(rate)}_k{code.info_bits}"] = lambda p=LinkDecodePlan(conv, "cuda"), t=llr: p(t, keys)
                shape[name]["viterbi"] = f"viterbi_m{m}_r{_name(rate)}_k{code.info_bits}"
    out = _measure(variants)
    for name, s in shape.items():
        work = s["rounds_per_wave"] * s["mean_iterations"] * s["edges"]
        out[name].update(s, ns_per_iteration_edge_of_a_wave=round(out[name]["median_us"] * 1e3 / work, 2),
                         soft_median_us=out[s["soft"]]["median_us"])
        if "viterbi" in s:
            out[name]["viterbi_median_us"] = out[s["viterbi"]]["median_us"]
    out["batch"], out["note"] = BATCH, NOTE
    return out


def section_i(a):
    from adafortitran_amd.hip_ops import LinkLdpcPlan, LinkSoftPlan
    from adafortitran_amd.linksim import LdpcConfig, LinkConfig
    cfg, ideal, est, keys, sigma, scale, one = _tensors()
    link = LinkConfig(cfg, 4)
    llr = LinkSoftPlan(link, "cuda")(ideal, est, keys, sigma, scale, one, want_llr=True)[1]
    variants, ran = {}, {}
    for iters in ITERS:
        code = LdpcConfig(link, "1/2", max_iters=iters)
        plan = LinkLdpcPlan(code, "cuda")
        variants[f"max_iters_{iters}"] = lambda p=plan: p(llr, keys)
        counts = plan(llr, keys)[0].sum(dim=0).tolist()
        ran[f"max_iters_{iters}"] = {"mean_iterations": round(counts[2] / (BATCH * code.blocks), 3),
                                     "bler": round(counts[1] / (BATCH * code.blocks), 4)}
    out = _measure(variants)
    for name, r in ran.items():
        out[name].update(r)
    out["case"], out["batch"], out["note"] = "m4_r12", BATCH, NOTE
    return out


def section_b(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import BlockErrorAccumulator, CodeConfig, LdpcBlockErrorAccumulator, LdpcConfig, LinkConfig
    from adafortitran_amd.lmmse import LmmseEstimator
    cfg = ChannelSimConfig()
    model = LmmseEstimator(cfg).to("cuda")
    ds, dop = 200.0, 800.0
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    codes = {}
    for m, rate in LINK_CASES:
        ldpc = LdpcConfig(LinkConfig(cfg, m), rate)
        codes[f"m{m}_r{_name(rate)}_ldpc"] = ldpc
        codes[f"m{m}_r{_name(rate)}_conv_k{ldpc.info_bits}"] = CodeConfig(LinkConfig(cfg, m), ldpc.info_bits, rate)
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, ls = torch.from_numpy(pack["h_ideal"]).cuda(), torch.from_numpy(pack["h_ls_full"]).cuda()
        pilots = torch.from_numpy(np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]])).cuda()
        meta = torch.from_numpy(pack["meta"])
        accs = {(c, which): (LdpcBlockErrorAccumulator if isinstance(code, LdpcConfig) else BlockErrorAccumulator)(code, "cuda", seed=1)
                for c, code in codes.items() for which in ("perfect", "lmmse", "ls")}
        for lo in range(0, a.frames, BATCH):
            sl = slice(lo, lo + BATCH)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (c, which), acc in accs.items():
                acc.update(est[which], ideal[sl], cols)
        row = {"snr_db": int(snr)}
        for (c, which), acc in accs.items():
            row[f"{c}_{which}"] = {"bler": round(acc.result(), 4), "throughput": round(acc.result_throughput(), 4)}
            if hasattr(acc, "result_iterations"):
                row[f"{c}_{which}"]["iterations"] = round(acc.result_iterations(), 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"frames_per_set": a.frames, "delay_spread_ns": ds, "doppler_hz": dop,
            "blocks_per_frame": {c: code.blocks for c, code in codes.items()}, "rows": rows}


SECTIONS = {"k": section_k, "i": section_i, "b": section_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_ldpc.json"))
    ap.add_argument("--sections", default="k,i,b")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("link_ldpc_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_ldpc_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_ldpc_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
