#!/usr/bin/env python3
"""What ordered successive cancellation on the two-stream link (linksim "the successive-cancellation link", aft_link_sic_f32) costs on
one MI355X, and what it measures beside the MMSE detector, the joint demapper and the genie bound.

    python tools/link_sic_bench.py [--out profiles/link_sic_bench.json] [--sections k,b] [--frames 128] [--device cuda|cpu] [--parent LIB]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   link_sic_kernel at m = 2, 4, 6 and 8 on 2 x 2 and 2 x 4, at one factor with its LLR output, as device-event time over many
      back-to-back launches, in alternating rounds with link_sm_kernel (aft_link_sm_f32, MMSE) and link_joint_kernel
      (aft_link_joint_f32) on the SAME tensors in the same process: the frames tools/link_joint_bench.py uses, at G = 32 groups and at
      G = 256 (one workgroup per compute unit).  All three read the same bytes, hash the same words and form the same eight sums; this
      kernel then adds one axis-LLR pass and four fused multiply-adds per element to the linear detector's work.  ``ratio_to_sm`` is
      recorded beside the joint kernel's; a description, not a target.  Not run with ``--device cpu``.
      With ``--parent LIB`` (a build of the parent commit's library, loaded beside this one) the linear and the joint kernel also run
      ONCE on that library on the same operands, and ``parent_bits`` records whether all their outputs are equal bit for bit;
  b   bit-error rate, achievable rate per stream (GMI, the best of the default factor grid) and LDPC block-error rate (rate 1/2) at
      16-QAM over the simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames, 2 x R with R = 2
      and 4, ``sic`` beside ``mmse`` and ``joint``: perfect channel knowledge, the LMMSE estimate and the interpolated LS estimate, and
      ``sic_propagation`` per SNR.  The ``genie`` bound (the SENT symbol is cancelled: host only) is ``link_sic_host(..., genie=True)`` on
      the same frames at R = 2: its bit-error rate and GMI.  Every case sees the same frames.  Reported, not asserted.  With
      ``--device cpu`` the float64 twins run in place of the kernels."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 400, "b": 900}     # seconds per child
GROUP_COUNTS = (32, 256)          # workgroups: a 128-frame batch at R = 2, and one per compute unit
BRANCHES = (2, 4)
KERNEL_BITS = (2, 4, 6, 8)
BITS = 4                          # section b: 16-QAM
DETECTORS = ("mmse", "sic", "joint")
GENIE_BRANCHES = 2

NOTE = ("device-event time per call over 100 back-to-back calls, 5 alternating rounds: the allocations of the outputs and the launch are "
        "inside it; the three kernels run at one factor with their LLR output on the same 2 G R frames (LMMSE estimates, the simulator's "
        "conditions drawn per frame, so the weights are mixed), G workgroups each")


def _parent_build(path):
    """The parent commit's build with the two older entry points typed from the binding's table: it lacks the new one, so
    ``_lib.load_path`` would refuse it."""
    import ctypes
    from adafortitran_amd import _abi
    lib = ctypes.CDLL(path)
    for name in ("aft_link_sm_f32", "aft_link_joint_f32", "aft_last_error", "aft_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _abi.SIGNATURES[name]
    return lib


def section_k(a):
    import torch
    from adafortitran_amd.hip_ops import LinkJointPlan, LinkSicPlan, LinkSmPlan
    from adafortitran_amd.linksim import LinkConfig
    from link_mrc_bench import _measure, _tensors              # the same frames, the same timing loop
    one = torch.ones(1, device="cuda")
    parent = _parent_build(os.path.abspath(a.parent)) if a.parent else None
    variants, same = {}, {}
    for G in GROUP_COUNTS:
        for R in BRANCHES:
            cfg, ideal, est, keys, sigma, scale = _tensors(G * 2 * R)
            s = scale.view(G, 2 * R).double()
            rho, lead = (s / s[:, :1]).float().reshape(-1), scale[::2 * R].contiguous()
            reg = (1.0 / lead.double()).float()
            for m in KERNEL_BITS:
                link = LinkConfig(cfg, m)
                with_reg, without = (ideal, est, keys, sigma, rho, lead, reg), (ideal, est, keys, sigma, rho, lead)
                plans = {"sic": (LinkSicPlan(link, "cuda", R), with_reg), "sm": (LinkSmPlan(link, "cuda", R), with_reg),
                         "joint": (LinkJointPlan(link, "cuda", R), without)}
                for tag, (p, t) in plans.items():
                    variants[f"{tag}_m{m}_r{R}_g{G}"] = lambda p=p, t=t: p(*t, one, want_llr=True)
                    if parent is not None and tag != "sic":     # the kernels that existed before: both builds once, every output's bits
                        mine, theirs = p(*t, one, want_llr=True), p(*t, one, want_llr=True, lib=parent)
                        same[f"{tag}_m{m}_r{R}_g{G}"] = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(mine, theirs))
    out = _measure(variants)
    for G in GROUP_COUNTS:
        for R in BRANCHES:
            for m in KERNEL_BITS:
                row, sm = out[f"sic_m{m}_r{R}_g{G}"], out[f"sm_m{m}_r{R}_g{G}"]["median_us"]
                row["sm_same_frames_median_us"], row["joint_same_frames_median_us"] = sm, out[f"joint_m{m}_r{R}_g{G}"]["median_us"]
                row["ratio_to_sm"] = round(row["median_us"] / sm, 4)
                row["joint_ratio_to_sm"] = round(row["joint_same_frames_median_us"] / sm, 4)
    if parent is not None:
        out["parent_bits"] = {"parent": os.path.basename(a.parent), "compared": len(same), "all_equal": all(same.values()),
                              "differing": sorted(k for k, v in same.items() if not v)}
    out["groups"], out["note"] = list(GROUP_COUNTS), NOTE
    return out


def section_b(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, frame_keys, make_pack
    from adafortitran_amd.linksim import (DEFAULT_FACTORS, LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator,
                                          link_sic_host, noise_sigma, sm_weights)
    from adafortitran_amd.lmmse import LmmseEstimator
    dev = a.device
    cfg = ChannelSimConfig()
    link = LinkConfig(cfg, BITS)
    code = LdpcConfig(link, "1/2")
    model = LmmseEstimator(cfg).to(dev)
    ds, dop = 200.0, 800.0
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    batch = min(128, a.frames)
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, ls = torch.from_numpy(pack["h_ideal"]).to(dev), torch.from_numpy(pack["h_ls_full"]).to(dev)
        pilots = torch.from_numpy(np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]])).to(dev)
        meta = torch.from_numpy(pack["meta"])
        accs = {(R, d, which): (LinkAccumulator(link, dev, seed=1, branches=R, streams=2, detector=d),
                                RateAccumulator(link, dev, seed=1, factors=DEFAULT_FACTORS, branches=R, streams=2, detector=d),
                                LdpcBlockErrorAccumulator(code, dev, seed=1, branches=R, streams=2, detector=d))
                for R in BRANCHES for d in DETECTORS for which in ("perfect", "lmmse", "ls")}
        genie = {which: [0, np.zeros(len(DEFAULT_FACTORS)), 0] for which in ("perfect", "lmmse", "ls")}     # bit errors, losses, rows
        for lo in range(0, a.frames, batch):
            sl = slice(lo, lo + batch)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            with torch.no_grad():
                est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (R, d, which), three in accs.items():
                for acc in three:
                    acc.update(est[which], ideal[sl], cols)
            # the genie bound on the host, on the same frames, keys and weights the accumulators form
            ids = np.rint(meta[sl, 0].numpy().astype(np.float64)).astype(np.int64)
            snrs = meta[sl, 1].numpy().reshape(-1)
            rho, scale, reg = sm_weights(snrs, 0.0, GENIE_BRANCHES, 2, "mmse")
            H = ideal[sl].cpu().numpy()
            for which, e in est.items():
                E = H if e is None else e.cpu().numpy()
                counts, loss, _, _ = link_sic_host(link, frame_keys(1, ids), H, E, noise_sigma(snrs), rho, scale, reg, GENIE_BRANCHES, 2,
                                                   DEFAULT_FACTORS, genie=True)
                genie[which][0] += int(counts[..., 0].sum())
                genie[which][1] += loss.sum(axis=(0, 1))
                genie[which][2] += counts.shape[0] * counts.shape[1]
        row = {"snr_db": int(snr)}
        for (R, d, which), (hard, rate, bler) in accs.items():
            row[f"2x{R}_{d}_{which}"] = {"ber": round(hard.result(), 6), "gmi_per_stream": round(rate.result_gmi(), 4),
                                         "ldpc_bler": round(bler.result(), 4), "ldpc_iterations": round(bler.result_iterations(), 3)}
            if d == "sic":
                row[f"2x{R}_{d}_{which}"]["propagation"] = [round(v, 5) for v in hard.sic_propagation()]
        for which, (errors, losses, n) in genie.items():
            row[f"2x{GENIE_BRANCHES}_genie_{which}"] = {"ber": round(errors / (n * link.bits_per_frame), 6),
                                                        "gmi_per_stream": round(float(max(BITS - losses / (n * link.data_elements))), 4)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"device": dev, "frames_per_set": a.frames, "bits_per_symbol": BITS, "ldpc": "rate 1/2, n = 1536", "blocks_per_stream_frame": code.blocks,
            "delay_spread_ns": ds, "doppler_hz": dop, "propagation": "share detected in swapped order, first decision's symbol-error rate, "
            "share of first-decision errors followed by a symbol error of the other stream", "genie": "link_sic_host(genie=True), float64, host",
            "rows": rows}


SECTIONS = {"k": section_k, "b": section_b}


def main():
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_sic_bench.json"))
    ap.add_argument("--sections", default="k,b")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"), help="cpu: section b on the float64 twins; section k is skipped")
    ap.add_argument("--parent", default="", help="section k: the parent commit's library, to compare the bits of the two older kernels with")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.frames < 1 or a.frames % (128 if a.frames > 128 else 2 * max(BRANCHES)):
        ap.error("--frames: a multiple of 8 up to 128, or a multiple of 128")
    if a.child:
        import torch
        if a.device == "cuda" and not torch.cuda.is_available():
            print("link_sic_bench.py: no GPU; --device cpu runs the twins", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_sic_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        if name == "k" and a.device == "cpu":
            continue
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames), "--device", a.device, "--parent", a.parent]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_sic_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
