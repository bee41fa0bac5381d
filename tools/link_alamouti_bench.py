#!/usr/bin/env python3
"""What transmit diversity on the link (linksim "the transmit-diversity link", aft_link_alamouti_f32) costs on one MI355X, and what it
measures.

    python tools/link_alamouti_bench.py [--out profiles/link_alamouti_bench.json] [--sections k,b,f] [--frames 128] [--device cuda|cpu]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the Alamouti kernel at 2 x 1, 2 x 2 and 2 x 4 for both pairings at m = 4 and 8 on 128 frames of the default grid (the bench's
      batch: 64, 32 and 16 groups), at one factor with its LLR output, as device-event time over many back-to-back launches, in
      alternating rounds with the combiner kernel (aft_link_mrc_f32, branches = 2 R, one factor, with its LLR output) on the SAME
      tensors.  Both read the same bytes and write the same LLRs; the combiner makes 2 R noise draws per element, this kernel R.  The
      same tree and the same process: a description, not a target.  Skipped on a CPU device;
  b   bit-error rate, achievable rate (GMI, the best of the default factor grid) and LDPC block-error rate (rate 1/2) at 16-QAM over
      the simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames: 2 x 1 Alamouti in both
      pairings beside 1 x 1 and 1 x 2 maximum-ratio combining on the same frames at EQUAL TOTAL POWER -- the Alamouti link's data is
      evaluated 3.01 dB below the set's SNR (each of its two antennas sends half the power); its per-antenna estimates are the set's,
      from orthogonal pilots at the set's SNR -- with perfect channel knowledge, the LMMSE estimate and the interpolated LS estimate;
  f   the figure the link exists for: with perfect channel knowledge and no noise to speak of (120 dB) the bit-error rate that
      channel variation inside a pair leaves, per pairing at 16- and 64-QAM, over the simulator's Doppler bins (at its smallest delay
      spread) and over its delay-spread bins (at its smallest Doppler), 2 x 1 on the groups of ``antennas=(1, 2)``.
``--device cpu`` runs the float64 twins in b and f.  Reported, not asserted."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 240, "b": 540, "f": 420}     # seconds per child
FRAMES = 128                      # section k: the bench's batch
BRANCHES = (1, 2, 4)
KERNEL_BITS = (4, 8)
BITS = 4                          # section b: 16-QAM
FLOOR_BITS = (4, 6)
POWER_SPLIT_DB = 3.0103           # two antennas at half the power each
NOISE_FREE_DB = 120.0

NOTE = ("device-event time per call over 100 back-to-back calls, 5 alternating rounds: the allocations of the outputs and the launch are "
        "inside it; both kernels run at one factor with their LLR output on the same 128 frames (LMMSE estimates, the simulator's "
        "conditions drawn per frame, so the weights are mixed) as 128 / (2 R) groups: the Alamouti kernel at R receive antennas, the "
        "combiner at branches = 2 R")


def section_k(a):
    import torch
    from adafortitran_amd.hip_ops import LinkAlamoutiPlan, LinkMrcPlan
    from adafortitran_amd.linksim import PAIRINGS, LinkConfig
    from link_mrc_bench import _measure, _tensors  # the same frames, the same timing loop
    if a.device != "cuda":
        return {"skipped": "the kernel runs on a HIP device"}
    one = torch.ones(1, device="cuda")
    cfg, ideal, est, keys, sigma, scale = _tensors(FRAMES)
    variants = {}
    for R in BRANCHES:
        s = scale.view(-1, 2 * R).double()
        rho, lead = (s / s[:, :1]).float().reshape(-1), scale[::2 * R].contiguous()
        t = (ideal, est, keys, sigma, rho, lead)
        for m in KERNEL_BITS:
            link = LinkConfig(cfg, m)
            for pairing in PAIRINGS:
                variants[f"alamouti_{pairing}_m{m}_2x{R}"] = lambda p=LinkAlamoutiPlan(link, "cuda", R, pairing), t=t: p(*t, one, want_llr=True)
            variants[f"mrc_m{m}_r{2 * R}"] = lambda p=LinkMrcPlan(link, "cuda", 2 * R), t=t: p(*t, one, want_llr=True)
    out = _measure(variants)
    worst = 0.0
    for R in BRANCHES:
        for m in KERNEL_BITS:
            for pairing in PAIRINGS:
                row = out[f"alamouti_{pairing}_m{m}_2x{R}"]
                row["mrc_same_tensors_median_us"] = out[f"mrc_m{m}_r{2 * R}"]["median_us"]
                row["ratio_to_mrc"] = round(row["median_us"] / row["mrc_same_tensors_median_us"], 4)
                worst = max(worst, row["ratio_to_mrc"])
    out["frames"], out["largest_ratio_to_mrc"], out["note"] = FRAMES, worst, NOTE
    return out


def _estimates(cfg, pack, device):
    """(ideal, {"perfect": None, "lmmse": .., "ls": ..}, meta columns) of a pack on ``device``."""
    import numpy as np
    import torch
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    pilots = np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]])
    meta = torch.from_numpy(pack["meta"])
    cols = tuple(meta[:, k:k + 1] for k in range(5)) + (None,)
    if device == "cuda":
        from adafortitran_amd.lmmse import LmmseEstimator
        lmmse = LmmseEstimator(cfg).to("cuda")(torch.from_numpy(pilots).cuda(), cols)
    else:
        from adafortitran_amd.lmmse import lmmse_estimate_host
        lmmse = torch.from_numpy(lmmse_estimate_host(cfg, pilots, pack["meta"][:, 1:4]).astype(np.complex64))
    to = lambda v: torch.from_numpy(v).to(device)  # noqa: E731
    return to(pack["h_ideal"]), {"perfect": None, "lmmse": lmmse, "ls": to(pack["h_ls_full"])}, cols


def section_b(a):
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import (DEFAULT_FACTORS, PAIRINGS, LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig,
                                          RateAccumulator)
    cfg = ChannelSimConfig()
    link = LinkConfig(cfg, BITS)
    code = LdpcConfig(link, "1/2")
    ds, dop = 200.0, 800.0
    links = {"1x1_mrc": dict(branches=1), "1x2_mrc": dict(branches=2),
             **{f"2x1_alamouti_{p}": dict(branches=1, tx_diversity=p) for p in PAIRINGS}}
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, est, cols = _estimates(cfg, pack, a.device)
        row = {"snr_db": int(snr)}
        for name, kw in links.items():
            data_snr = float(snr) - (POWER_SPLIT_DB if "tx_diversity" in kw else 0.0)
            for which, e in est.items():
                hard = LinkAccumulator(link, a.device, seed=1, **kw)
                rate = RateAccumulator(link, a.device, seed=1, factors=DEFAULT_FACTORS, **kw)
                bler = LdpcBlockErrorAccumulator(code, a.device, seed=1, **kw)
                for acc in (hard, rate, bler):
                    acc.update(e, ideal, cols, snr_db=data_snr)
                row[f"{name}_{which}"] = {"ber": round(hard.result(), 6), "gmi": round(rate.result_gmi(), 4),
                                          "ldpc_bler": round(bler.result(), 4), "ldpc_iterations": round(bler.result_iterations(), 3)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"frames_per_set": a.frames, "bits_per_symbol": BITS, "ldpc": "rate 1/2, n = 1536", "blocks_per_frame": code.blocks,
            "delay_spread_ns": ds, "doppler_hz": dop, "alamouti_data_snr_offset_db": -POWER_SPLIT_DB, "rows": rows}


def section_f(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import PAIRINGS, LinkAccumulator, LinkConfig
    cfg = ChannelSimConfig(antennas=(1, 2))
    out = {"frames_per_set": a.frames, "snr_db": NOISE_FREE_DB, "doppler": [], "delay_spread": []}

    def floors(**pinned):
        pack = make_pack(cfg, a.frames, seed=7, snr_db=float(cfg.snr_db[-1]), **pinned)
        ideal = torch.from_numpy(pack["h_ideal"]).to(a.device)
        meta = torch.from_numpy(pack["meta"])
        cols = tuple(meta[:, k:k + 1] for k in range(5)) + (None,)
        row = dict(pinned)
        for m in FLOOR_BITS:
            for pairing in PAIRINGS:
                acc = LinkAccumulator(LinkConfig(cfg, m), a.device, seed=1, branches=1, tx_diversity=pairing)
                acc.update(None, ideal, cols, snr_db=NOISE_FREE_DB)
                row[f"ber_m{m}_{pairing}"] = acc.result()
        print(json.dumps(row), file=sys.stderr)
        return row

    for dop in cfg.doppler_hz:
        out["doppler"].append(floors(delay_spread_ns=float(cfg.delay_spread_ns[0]), doppler_hz=float(dop)))
    for ds in cfg.delay_spread_ns:
        out["delay_spread"].append(floors(delay_spread_ns=float(ds), doppler_hz=float(cfg.doppler_hz[0])))
    return out


SECTIONS = {"k": section_k, "b": section_b, "f": section_f}


def main():
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_alamouti_bench.json"))
    ap.add_argument("--sections", default="k,b,f")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.frames < 2 or a.frames % 2:
        ap.error("--frames: a multiple of 2")
    if a.child:
        import torch
        if a.device == "cuda" and not torch.cuda.is_available():
            print("link_alamouti_bench.py: no GPU; nothing is measured without one (--device cpu runs the twins)", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_alamouti_bench.py", "grid": [120, 14], "pilots": [12, 2], "device": a.device}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames), "--device", a.device]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_alamouti_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
