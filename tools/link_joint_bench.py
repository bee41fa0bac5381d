#!/usr/bin/env python3
"""What joint max-log detection on the two-stream link (linksim "the joint link", aft_link_joint_f32) costs on one MI355X, and what it
measures beside the MMSE detector.

    python tools/link_joint_bench.py [--out profiles/link_joint_bench.json] [--sections k,b] [--frames 128] [--base-lib PATH]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   link_joint_kernel at m = 2, 4, 6 and 8 on 2 x 2 and 2 x 4, at one factor with its LLR output, as device-event time over many
      back-to-back launches, in alternating rounds with link_sm_kernel (aft_link_sm_f32, MMSE) on the SAME frames: at G = 32 groups
      (a 128-frame batch at R = 2: 32 workgroups on 256 compute units) and at G = 256 (one workgroup per compute unit).  Both read
      the same bytes, hash the same words and form the same eight sums; the joint kernel then evaluates 2 M candidates per data
      element where the linear one runs two L-level demappers.  The same tree and the same process: a description, not a target.
      With ``--base-lib PATH`` (another build of the library with the same ABI, loaded beside this one) every variant also runs on
      that library in the same alternating rounds, and ``vs_base`` holds this build's median over the other's per variant;
  b   bit-error rate, achievable rate per stream (GMI, the best of the default factor grid) and LDPC block-error rate (rate 1/2) at
      16-QAM over the simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames, 2 x R with R = 2
      and 4, joint beside MMSE: perfect channel knowledge, the LMMSE estimate (on the device) and the interpolated LS estimate.
      Every case sees the same frames.  Reported, not asserted."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from link_mrc_bench import _measure, _tensors  # noqa: E402  the same frames, the same timing loop

LIMITS = {"k": 300, "b": 540}     # seconds per child
GROUP_COUNTS = (32, 256)          # workgroups: a 128-frame batch at R = 2, and one per compute unit
BRANCHES = (2, 4)
KERNEL_BITS = (2, 4, 6, 8)
BITS = 4                          # section b: 16-QAM
DETECTORS = ("mmse", "joint")

NOTE = ("device-event time per call over 100 back-to-back calls, 5 alternating rounds: the allocations of the outputs and the launch are "
        "inside it; both kernels run at one factor with their LLR output on the same 2 G R frames (LMMSE estimates, the simulator's "
        "conditions drawn per frame, so the weights are mixed), G workgroups each; candidates_per_element = 2 M per stream pair")


def section_k(a):
    import torch
    from adafortitran_amd import _lib
    from adafortitran_amd.hip_ops import LinkJointPlan, LinkSmPlan
    from adafortitran_amd.linksim import LinkConfig
    one = torch.ones(1, device="cuda")
    libs = {"": None, **({"_base": _lib.load_path(a.base_lib)} if a.base_lib else {})}      # None: this tree's library
    variants = {}
    for G in GROUP_COUNTS:
        for R in BRANCHES:
            cfg, ideal, est, keys, sigma, scale = _tensors(G * 2 * R)
            s = scale.view(G, 2 * R).double()
            rho, lead = (s / s[:, :1]).float().reshape(-1), scale[::2 * R].contiguous()
            reg = (1.0 / lead.double()).float()
            for m in KERNEL_BITS:
                link = LinkConfig(cfg, m)
                for tag, lib in libs.items():
                    variants[f"joint_m{m}_r{R}_g{G}{tag}"] = \
                        lambda p=LinkJointPlan(link, "cuda", R), t=(ideal, est, keys, sigma, rho, lead), lib=lib: p(*t, one, want_llr=True, lib=lib)
                    variants[f"sm_m{m}_r{R}_g{G}{tag}"] = \
                        lambda p=LinkSmPlan(link, "cuda", R), t=(ideal, est, keys, sigma, rho, lead, reg), lib=lib: p(*t, one, want_llr=True, lib=lib)
    out = _measure(variants)
    if a.base_lib:
        ratios = {k: round(out[k]["median_us"] / out.pop(k + "_base")["median_us"], 4) for k in list(out) if not k.endswith("_base")}
        out["vs_base"] = {"base_lib": os.path.basename(a.base_lib), "median_over_base_median": ratios,
                          "largest": max(ratios.values()), "smallest": min(ratios.values())}
    data = 1680 - 24                                             # data elements of the default grid
    for G in GROUP_COUNTS:
        for R in BRANCHES:
            for m in KERNEL_BITS:
                row = out[f"joint_m{m}_r{R}_g{G}"]
                row["sm_same_frames_median_us"] = out[f"sm_m{m}_r{R}_g{G}"]["median_us"]
                row["ratio_to_sm"] = round(row["median_us"] / row["sm_same_frames_median_us"], 4)
                row["candidates_per_element"] = 2 << m
                row["ps_per_candidate"] = round(row["median_us"] * 1e6 / (G * data * (2 << m)), 3)
    out["groups"], out["note"] = list(GROUP_COUNTS), NOTE
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
    batch = min(128, a.frames)
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, ls = torch.from_numpy(pack["h_ideal"]).cuda(), torch.from_numpy(pack["h_ls_full"]).cuda()
        pilots = torch.from_numpy(np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]])).cuda()
        meta = torch.from_numpy(pack["meta"])
        accs = {(R, d, which): (LinkAccumulator(link, "cuda", seed=1, branches=R, streams=2, detector=d),
                                RateAccumulator(link, "cuda", seed=1, factors=DEFAULT_FACTORS, branches=R, streams=2, detector=d),
                                LdpcBlockErrorAccumulator(code, "cuda", seed=1, branches=R, streams=2, detector=d))
                for R in BRANCHES for d in DETECTORS for which in ("perfect", "lmmse", "ls")}
        for lo in range(0, a.frames, batch):
            sl = slice(lo, lo + batch)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (R, d, which), three in accs.items():
                for acc in three:
                    acc.update(est[which], ideal[sl], cols)
        row = {"snr_db": int(snr)}
        for (R, d, which), (hard, rate, bler) in accs.items():
            row[f"2x{R}_{d}_{which}"] = {"ber": round(hard.result(), 6), "gmi_per_stream": round(rate.result_gmi(), 4),
                                         "ldpc_bler": round(bler.result(), 4), "ldpc_iterations": round(bler.result_iterations(), 3)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"frames_per_set": a.frames, "bits_per_symbol": BITS, "ldpc": "rate 1/2, n = 1536", "blocks_per_stream_frame": code.blocks,
            "delay_spread_ns": ds, "doppler_hz": dop, "rows": rows}


SECTIONS = {"k": section_k, "b": section_b}


def main():
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_joint_bench.json"))
    ap.add_argument("--sections", default="k,b")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--base-lib", default="", help="section k: another build of the library to time every variant on as well")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.frames < 1 or a.frames % (128 if a.frames > 128 else 2 * max(BRANCHES)):
        ap.error("--frames: a multiple of 8 up to 128, or a multiple of 128")
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("link_joint_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_joint_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames), "--base-lib", a.base_lib]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_joint_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
