#!/usr/bin/env python3
"""What antenna correlation in the channel simulator (chansim "Kronecker frame groups", aft_channel_sim_group_f32) costs on one MI355X,
and what it does to the links.

    python tools/chansim_corr_bench.py [--out profiles/chansim_corr_bench.json] [--sections k,p,s] [--frames 256] [--parent LIB]
                                       [--device cuda|cpu]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the grouped kernel at G = 2, 4, 8 and 16 (antennas (2,1), (2,2), (4,2), (8,2), rho 0.7 wherever a dimension has two antennas)
      beside the ungrouped kernel on the SAME number of default-grid frames, 128 (half a wave of workgroups) and 4096 (16 workgroups
      per compute unit): device-event time over many back-to-back calls of the entry point on preallocated outputs, in alternating
      rounds.  Only the gain pass grows with G, by (G + 1) / 2 sources per frame on average;
  p   the ungrouped kernel of this build against the same entry point of another build of the library (``--parent``: the commit before
      the grouped instantiation), interleaved on the same outputs, in both orders, and a bit comparison of their outputs on three
      grids; skipped without --parent;
  s   BER, GMI and LDPC block-error rate over the simulator's SNR grid at a mid delay spread and Doppler for perfect channel knowledge,
      the LMMSE estimate and the interpolated LS estimate, at rho in {0, 0.5, 0.9} (receive side; both sides for the two-stream links):
      maximum-ratio combining with R = 2 and R = 4, and 2 x 2 and 2 x 4 multiplexing with MMSE and joint detection.  16-QAM, rate-1/2
      LDPC.  ``--device cpu`` runs the float64 twins instead (the record says so: use a reduced --frames).  Reported, not asserted."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 240, "p": 240, "s": 900}     # seconds per child
KERNEL_FRAMES = (128, 4096)
GROUPS = {2: ((2, 1), 0.7, None), 4: ((2, 2), 0.7, 0.7), 8: ((4, 2), 0.7, 0.7), 16: ((8, 2), 0.7, 0.7)}
RHOS = (0.0, 0.5, 0.9)
BITS = 4
NOTE = ("device-event time per call over 200 back-to-back calls of the entry point on preallocated outputs, 7 alternating rounds: the "
        "ctypes call and the launch are inside it, no allocation is")


def _stats(values):
    return {"median_us": round(statistics.median(values), 4), "min_us": round(min(values), 4), "max_us": round(max(values), 4),
            "spread_us": round(max(values) - min(values), 4)}


def _measure(variants, reps=200, rounds=7):
    import torch
    from train_loader_bench import _event_us
    torch.cuda.synchronize()
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            us[k].append(_event_us(fn, reps))
    return {k: _stats(v) for k, v in us.items()}


def _call(cfg, frames, lib=None):
    """``(fn, outputs)``: one call of the configuration's entry point for ``frames`` frames of seed 1 into outputs allocated once."""
    import torch
    from adafortitran_amd import _lib
    from adafortitran_amd.hip_ops import ChannelSimPlan
    plan = ChannelSimPlan(cfg, "cuda")
    lib = lib or _lib.load()
    outs = (torch.empty((frames, *cfg.ofdm), dtype=torch.complex64, device="cuda"),
            torch.empty((frames, *cfg.pilot), dtype=torch.complex64, device="cuda"), torch.empty((frames, 3), device="cuda"))
    ptr = [t.data_ptr() for t in outs]
    stream = _lib.current_stream_ptr(outs[0].device)
    if plan.group > 1:
        def fn():
            _lib.check(lib.aft_channel_sim_group_f32(plan.sim, *plan.antennas, plan.mix.ctypes.data, 1, 0, 0, 1, 1 << 40, frames, *ptr,
                                                     stream), lib)
    else:
        def fn():
            _lib.check(lib.aft_channel_sim_f32(plan.sim, 1, 0, 0, 1, 1 << 40, frames, *ptr, stream), lib)
    fn.keep = plan                                                               # the struct and the packed mix outlive the calls
    return fn, outs


def section_k(a):
    from adafortitran_amd.chansim import ChannelSimConfig
    out = {"note": NOTE}
    for frames in KERNEL_FRAMES:
        variants = {"ungrouped": _call(ChannelSimConfig(), frames)[0]}
        for G, (antennas, rx, tx) in GROUPS.items():
            variants[f"grouped_G{G}"] = _call(ChannelSimConfig(antennas=antennas, rx_correlation=rx, tx_correlation=tx), frames)[0]
        got = _measure(variants)
        base = got["ungrouped"]["median_us"]
        for G in GROUPS:
            got[f"grouped_G{G}"].update(ratio_to_ungrouped=round(got[f"grouped_G{G}"]["median_us"] / base, 3),
                                        mean_sources_per_frame=(G + 1) / 2)
        out[f"frames_{frames}"] = got
    return out


def _parent_build(path):
    """Another build of the library with ``aft_channel_sim_f32`` typed from the binding's table: the entry point kept its signature,
    meaning and bits across the ABI bump, which is what this section measures."""
    import ctypes
    from adafortitran_amd import _abi
    lib = ctypes.CDLL(path)
    for name in ("aft_channel_sim_f32", "aft_last_error", "aft_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _abi.SIGNATURES[name]
    return lib


def section_p(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    parent = _parent_build(os.path.abspath(a.parent))
    same = {}
    for name, cfg in (("default_120x14", ChannelSimConfig()), ("long_72x80", ChannelSimConfig(ofdm=(72, 80), pilot=(6, 4))),
                      ("odd_30x7", ChannelSimConfig(ofdm=(30, 7), pilot=(3, 1)))):
        (here, out_here), (there, out_there) = _call(cfg, 256), _call(cfg, 256, lib=parent)
        here(), there()
        torch.cuda.synchronize()
        same[name] = bool(all(torch.equal(torch.view_as_real(x).view(torch.int32) if x.is_complex() else x.view(torch.int32),
                                          torch.view_as_real(y).view(torch.int32) if y.is_complex() else y.view(torch.int32))
                              for x, y in zip(out_here, out_there)))
    out = {"outputs_identical": same, "parent_abi": parent.aft_version(), "note": NOTE}
    for frames in KERNEL_FRAMES:
        variants = {"this_build": _call(ChannelSimConfig(), frames)[0], "parent_build": _call(ChannelSimConfig(), frames, lib=parent)[0]}
        # twice, the second time in the other order inside a round: what follows what is not the build's
        orders = {"this_build_first": _measure(variants), "parent_build_first": _measure(dict(reversed(list(variants.items()))))}
        this, par = [o["this_build"] for o in orders.values()], [o["parent_build"] for o in orders.values()]
        lo, hi = min(p["min_us"] for p in par), max(p["max_us"] for p in par)
        out[f"frames_{frames}"] = dict(orders, median_difference_us=[round(t["median_us"] - p["median_us"], 4) for t, p in zip(this, par)],
                                       parent_range_us=[lo, hi], parent_spread_us=round(hi - lo, 4),
                                       within_the_parents_spread=bool(all(t["median_us"] <= hi for t in this)))
    return out


def _frames(cfg, n, seed, device):
    """``(ideal, pilots, meta columns, ls)`` of frames [0, n) on ``device``: the kernel's on a HIP device, the float64 twin's on the CPU;
    the LS estimate is the pilots interpolated on the host either way."""
    import numpy as np
    import torch
    from adafortitran_amd.chansim import frame_conditions, ls_interpolate, simulate_frames_host
    if device == "cuda":
        from adafortitran_amd.hip_ops import ChannelSimPlan
        ideal, pilots, _ = ChannelSimPlan(cfg, "cuda")(seed, 0, 0, 1, 1 << 40, n)
    else:
        ideal, pilots = (torch.from_numpy(x.astype(np.complex64)) for x in simulate_frames_host(cfg, seed, np.arange(n))[:2])
    cond = frame_conditions(cfg, seed, np.arange(n))
    meta = torch.from_numpy(np.concatenate([np.arange(n, dtype=np.float32)[:, None], cond, np.zeros((n, 1), np.float32)], axis=1))
    ls = torch.from_numpy(ls_interpolate(cfg, pilots.cpu().numpy())).to(ideal.device)
    return ideal, pilots, meta, ls


def section_s(a):
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.linksim import DEFAULT_FACTORS, LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig, RateAccumulator
    from adafortitran_amd.lmmse import LmmseEstimator
    dev, ds, dop = a.device, 200.0, 800.0
    base = ChannelSimConfig()
    model = LmmseEstimator(base).to(dev)                        # per-antenna: the tables know nothing of the correlation
    # receiver -> (antennas, accumulator arguments): the group of the link is the group of the simulator
    receivers = {"mrc_R2": ((2, 1), dict(branches=2)), "mrc_R4": ((4, 1), dict(branches=4))}
    for R in (2, 4):
        for d in ("mmse", "joint"):
            receivers[f"2x{R}_{d}"] = ((R, 2), dict(branches=R, streams=2, detector=d))
    batch = min(128, a.frames)
    rows = []
    for rho in RHOS:
        for snr in base.snr_db:
            row = {"rho": rho, "snr_db": int(snr)}
            made = {}
            for name, (antennas, kw) in receivers.items():
                if antennas not in made:
                    cfg = ChannelSimConfig(snr_db=(snr,), delay_spread_ns=(ds,), doppler_hz=(dop,), antennas=antennas,
                                           rx_correlation=rho or None, tx_correlation=(rho or None) if antennas[1] > 1 else None)
                    made[antennas] = (cfg, _frames(cfg, a.frames, 100 + int(snr), dev))
                cfg, (ideal, pilots, meta, ls) = made[antennas]
                link = LinkConfig(cfg, BITS)
                code = LdpcConfig(link, "1/2")
                for which in ("perfect", "lmmse", "ls"):
                    accs = (LinkAccumulator(link, dev, seed=1, **kw), RateAccumulator(link, dev, seed=1, factors=DEFAULT_FACTORS, **kw),
                            LdpcBlockErrorAccumulator(code, dev, seed=1, **kw))
                    for lo in range(0, a.frames, batch):
                        sl = slice(lo, lo + batch)
                        cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
                        est = None if which == "perfect" else ls[sl] if which == "ls" else model(pilots[sl], cols)
                        for acc in accs:
                            acc.update(est, ideal[sl], cols)
                    row[f"{name}_{which}"] = {"ber": round(accs[0].result(), 6), "gmi": round(accs[1].result_gmi(), 4),
                                              "ldpc_bler": round(accs[2].result(), 4)}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    return {"frames_per_set": a.frames, "made_by": "the float64 CPU twins" if dev == "cpu" else "the device kernels", "bits_per_symbol": BITS,
            "ldpc": "rate 1/2, n = 1536", "delay_spread_ns": ds, "doppler_hz": dop, "rows": rows}


SECTIONS = {"k": section_k, "p": section_p, "s": section_s}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chansim_corr_bench.json"))
    ap.add_argument("--sections", default="k,p,s")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--parent", default="", help="another build of the library for section p")
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"), help="section s: the device kernels or the float64 CPU twins")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.frames % 16 or (a.frames > 128 and a.frames % 128):
        ap.error("--frames must be a multiple of 16, and of 128 beyond 128")
    if a.child:
        if a.child != "s" or a.device == "cuda":
            import torch
            if not torch.cuda.is_available():
                print("chansim_corr_bench.py: no GPU; only section s with --device cpu runs without one", file=sys.stderr)
                return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/chansim_corr_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        if name == "p" and not a.parent:
            record["p"] = "skipped: no --parent library given"
            continue
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames), "--parent", a.parent, "--device", a.device]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"chansim_corr_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
