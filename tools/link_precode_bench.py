#!/usr/bin/env python3
"""What closed-loop precoding on the link (linksim "the closed-loop link", aft_link_precoded_f32) costs on one MI355X, and what it
measures.

    python tools/link_precode_bench.py [--out profiles/link_precode_bench.json] [--sections k,b,f] [--frames 128] [--device cuda|cpu]
                                       [--trace DIR]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the precoding kernel on 4096 frames of the default grid at R = 1, 2 and 4 receive antennas (2048, 1024 and 512 groups), m = 2
      and 6 and subbands of B = 1, 12 and S = 120 subcarriers, at one factor with its LLR output, as device-event time over many
      back-to-back launches, in alternating rounds with the Alamouti kernel (aft_link_alamouti_f32, time pairing, the same R) on the
      SAME tensors.  Both read the same H and write the same LLRs; this kernel reads every estimate twice, once for the selection and
      once in the element walk, and writes the PMIs.  The same tree and the same process: a description, not a target.  Skipped on a
      CPU device;
  p   for the profiler (``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/link_precode_bench.py --child
      p``): section k's variants in its order, ``TRACE_CALLS`` launches of each and nothing else.  A later run with ``--trace DIR``
      reads the trace's dispatches of the two kernels in their order of start, cuts them into the variants' runs and records each
      variant's KERNEL time (median of its dispatches) beside section k's call time; without ``--trace`` the record says that the
      kernel time was not measured;
  b   bit-error rate and achievable rate (GMI, the best of the default factor grid) at 16-QAM over the simulator's SNR grid at a mid
      delay spread and Doppler, make_pack sets of ``--frames`` frames: 2 x 1 precoded (B = 12) beside 2 x 1 Alamouti (time pairing) and
      the single-antenna link on the same frames at EQUAL TOTAL POWER -- the two-antenna links' data is evaluated 3.01 dB below the
      set's SNR (each antenna sends half the power); the per-antenna estimates are the set's, from orthogonal pilots at the set's SNR
      -- with perfect channel knowledge and the LMMSE estimate (no trained checkpoint ships with the tree: not measured);
  f   the figure the link exists for: the share of subbands whose PMI from the LMMSE estimate differs from the PMI from the true
      channel (a second launch with ``est = ideal``), 2 x 1 on the groups of ``antennas=(1, 2)``, B = 1, 12 and 120, per SNR of the
      simulator's grid (at a mid delay spread) and per delay-spread bin (at 20 dB), at a mid Doppler.
``--device cpu`` runs the float64 twins in b and f.  Reported, not asserted."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 300, "p": 300, "b": 540, "f": 420}     # seconds per child
FRAMES = 4096                     # sections k and p
BRANCHES = (1, 2, 4)
KERNEL_BITS = (2, 6)
SUBBANDS = (1, 12, 120)
TRACE_CALLS = 50
BITS = 4                          # section b: 16-QAM
LINK_SUBBAND = 12
POWER_SPLIT_DB = 3.0103           # two antennas at half the power each

NOTE = ("device-event time per call over 100 back-to-back calls, 5 alternating rounds: the allocations of the outputs and the launch are "
        "inside it; both kernels run at one factor with their LLR output on the same 4096 frames (LMMSE estimates, the simulator's "
        "conditions drawn per frame, so the weights are mixed) as 4096 / (2 R) groups")


def _variants():
    """Section k's and p's launches in one fixed order: name -> a call."""
    import torch
    from adafortitran_amd.hip_ops import LinkAlamoutiPlan, LinkPrecodedPlan
    from adafortitran_amd.linksim import LinkConfig
    from link_mrc_bench import _tensors  # the same frames
    one = torch.ones(1, device="cuda")
    cfg, ideal, est, keys, sigma, scale = _tensors(FRAMES)
    variants = {}
    for R in BRANCHES:
        s = scale.view(-1, 2 * R).double()
        rho, lead = (s / s[:, :1]).float().reshape(-1), scale[::2 * R].contiguous()
        t = (ideal, est, keys, sigma, rho, lead)
        for m in KERNEL_BITS:
            link = LinkConfig(cfg, m)
            for B in SUBBANDS:
                variants[f"precoded_m{m}_2x{R}_b{B}"] = lambda p=LinkPrecodedPlan(link, "cuda", R, B), t=t: p(*t, one, want_llr=True)
            variants[f"alamouti_time_m{m}_2x{R}"] = lambda p=LinkAlamoutiPlan(link, "cuda", R, "time"), t=t: p(*t, one, want_llr=True)
    return variants


def _names():
    return [name for R in BRANCHES for m in KERNEL_BITS
            for name in (*(f"precoded_m{m}_2x{R}_b{B}" for B in SUBBANDS), f"alamouti_time_m{m}_2x{R}")]


def section_k(a):
    from link_mrc_bench import _measure  # the same timing loop
    if a.device != "cuda":
        return {"skipped": "the kernel runs on a HIP device"}
    out = _measure(_variants())
    worst = 0.0
    for R in BRANCHES:
        for m in KERNEL_BITS:
            for B in SUBBANDS:
                row = out[f"precoded_m{m}_2x{R}_b{B}"]
                row["alamouti_same_tensors_median_us"] = out[f"alamouti_time_m{m}_2x{R}"]["median_us"]
                row["ratio_to_alamouti"] = round(row["median_us"] / row["alamouti_same_tensors_median_us"], 4)
                worst = max(worst, row["ratio_to_alamouti"])
    out["frames"], out["largest_ratio_to_alamouti"], out["note"] = FRAMES, worst, NOTE
    return out


def section_p(a):
    import torch
    if a.device != "cuda":
        return {"skipped": "the kernel runs on a HIP device"}
    variants = _variants()
    assert list(variants) == _names()
    torch.cuda.synchronize()
    for fn in variants.values():
        for _ in range(TRACE_CALLS):
            fn()
        torch.cuda.synchronize()
    return {"calls_per_variant": TRACE_CALLS, "variants": list(variants)}


def kernel_times(trace_dir):
    """Section p's trace -> {variant: {"kernel_median_us", "kernel_min_us", "dispatches"}}: the dispatches of the two kernels in their
    order of start, ``TRACE_CALLS`` per variant in section p's order.  Raises where the trace does not hold exactly those."""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise RuntimeError(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                if "link_precoded_kernel" in name or "link_alamouti_kernel" in name:
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), name))
    rows.sort()
    names = _names()
    if len(rows) != TRACE_CALLS * len(names):
        raise RuntimeError(f"{len(rows)} dispatches of the two kernels in the trace, expected {TRACE_CALLS} x {len(names)}")
    out = {}
    for i, variant in enumerate(names):
        part = rows[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]
        kernel = "link_precoded_kernel" if variant.startswith("precoded") else "link_alamouti_kernel"
        if not all(kernel in r[2] for r in part):
            raise RuntimeError(f"the dispatches of {variant} are not all {kernel}")
        us = [(end - start) / 1e3 for start, end, _ in part[5:]]                  # the first five: warm-up
        out[variant] = {"kernel_median_us": round(statistics.median(us), 2), "kernel_min_us": round(min(us), 2), "dispatches": len(us)}
    for R in BRANCHES:
        for m in KERNEL_BITS:
            for B in SUBBANDS:
                row = out[f"precoded_m{m}_2x{R}_b{B}"]
                row["kernel_ratio_to_alamouti"] = round(row["kernel_median_us"] / out[f"alamouti_time_m{m}_2x{R}"]["kernel_median_us"], 4)
    return out


def section_b(a):
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import DEFAULT_FACTORS, LinkAccumulator, LinkConfig, RateAccumulator
    from link_alamouti_bench import _estimates
    cfg = ChannelSimConfig()
    link = LinkConfig(cfg, BITS)
    ds, dop = 200.0, 800.0
    links = {"1x1": dict(branches=1), "2x1_alamouti_time": dict(branches=1, tx_diversity="time"),
             f"2x1_precoded_b{LINK_SUBBAND}": dict(branches=1, precoding_subband=LINK_SUBBAND)}
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, est, cols = _estimates(cfg, pack, a.device)
        row = {"snr_db": int(snr)}
        for name, kw in links.items():
            data_snr = float(snr) - (POWER_SPLIT_DB if len(kw) > 1 else 0.0)
            for which in ("perfect", "lmmse"):
                hard = LinkAccumulator(link, a.device, seed=1, **kw)
                rate = RateAccumulator(link, a.device, seed=1, factors=DEFAULT_FACTORS, **kw)
                for acc in (hard, rate):
                    acc.update(est[which], ideal, cols, snr_db=data_snr)
                row[f"{name}_{which}"] = {"ber": round(hard.result(), 6), "gmi": round(rate.result_gmi(), 4)}
                if "precoding_subband" in kw:
                    row[f"{name}_{which}"]["pmi_histogram"] = hard.pmi_histogram()
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"frames_per_set": a.frames, "bits_per_symbol": BITS, "delay_spread_ns": ds, "doppler_hz": dop,
            "two_antenna_data_snr_offset_db": -POWER_SPLIT_DB, "trained_estimator": "not measured: no checkpoint ships with the tree",
            "rows": rows}


def section_f(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, frame_keys, make_pack
    from adafortitran_amd.linksim import LinkConfig, llr_scale, noise_sigma, precoding_pmi_host, precoding_weights
    from link_alamouti_bench import _estimates
    cfg = ChannelSimConfig(antennas=(1, 2))
    link = LinkConfig(cfg, BITS)
    dop = 800.0
    out = {"frames_per_set": a.frames, "doppler_hz": dop, "snr": [], "delay_spread": []}

    def shares(snr, ds):
        pack = make_pack(cfg, a.frames, seed=11, snr_db=float(snr), delay_spread_ns=float(ds), doppler_hz=dop)
        ideal, est, _ = _estimates(cfg, pack, a.device)
        n = ideal.shape[0]
        snrs = np.full(n, float(snr))
        rho, scale = precoding_weights(snrs, 0.0, 1)
        row = {"snr_db": float(snr), "delay_spread_ns": float(ds)}
        for B in SUBBANDS:
            if a.device == "cuda":
                from adafortitran_amd.hip_ops import LinkPrecodedPlan
                plan = LinkPrecodedPlan(link, "cuda", 1, B)
                dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
                rest = (dev(frame_keys(1, np.arange(n)).view(np.int64)), dev(noise_sigma(snrs).astype(np.float32)), dev(rho), dev(scale),
                        torch.ones(1, device="cuda"))
                chosen, best = plan(ideal, est["lmmse"], *rest)[3], plan(ideal, ideal, *rest)[3]
                differ = float((chosen != best).double().mean().item())
            else:
                chosen = precoding_pmi_host(link, est["lmmse"].numpy(), rho, 1, B)
                differ = float((chosen != precoding_pmi_host(link, ideal.numpy(), rho, 1, B)).mean())
            row[f"pmi_differs_b{B}"] = round(differ, 5)
        print(json.dumps(row), file=sys.stderr)
        return row

    for snr in cfg.snr_db:
        out["snr"].append(shares(snr, 200.0))
    for ds in cfg.delay_spread_ns:
        out["delay_spread"].append(shares(20.0, ds))
    return out


SECTIONS = {"k": section_k, "p": section_p, "b": section_b, "f": section_f}


def main():
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_precode_bench.json"))
    ap.add_argument("--sections", default="k,b,f")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--trace", default="", help="the directory of a rocprofv3 --kernel-trace run of --child p")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.frames < 2 or a.frames % 2:
        ap.error("--frames: a multiple of 2")
    if a.child:
        import torch
        if a.device == "cuda" and not torch.cuda.is_available():
            print("link_precode_bench.py: no GPU; nothing is measured without one (--device cpu runs the twins)", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_precode_bench.py", "grid": [120, 14], "pilots": [12, 2], "device": a.device}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames), "--device", a.device]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_precode_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
            record["stopped_at"], status = name, res.returncode
            break
        record[name] = json.loads(res.stdout.strip().splitlines()[-1])
    if a.trace:
        record["kernel_time"] = {"source": "rocprofv3 --kernel-trace of --child p, median over the dispatches of each variant after five",
                                 "frames": FRAMES, **kernel_times(a.trace)}
    else:
        record["kernel_time"] = "not measured: no --trace"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps(record))
    return status


if __name__ == "__main__":
    sys.exit(main())
