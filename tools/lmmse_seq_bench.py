#!/usr/bin/env python3
"""What the multi-slot LMMSE estimator (lmmse.LmmseEstimator(window=, horizon=), aft_lmmse_seq_f32) costs on one MI355X, and what it buys.

    python tools/lmmse_seq_bench.py [--out profiles/lmmse_seq_bench.json] [--sections k,n,h,m] [--frames 4096] [--parent LIB]
                                    [--device cuda|cpu]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the kernel at W = 1, 2, 4, 8 on `--frames` frames of the default grid in sequences of K = 8 slots, next to aft_lmmse_f32 on the
      same pilots: device-event time per call over back-to-back calls, in alternating rounds (the warm-up and repeat rules of
      tools/lmmse_bench.py).  With ``--parent LIB`` aft_lmmse_f32 of that build runs in the same rounds and its bits are compared.
      Needs a GPU;
  n   NMSE on the steady slots (those with a full window) for W = 1, 2, 4, 8 over SNR 0 .. 30 dB at 50 / 200 / 800 Hz, 200 ns, with
      the closed form (lmmse_predicted_mse) next to each value;
  h   NMSE of the h-ahead prediction, h = 1, 2, 4, with W = 4 at 10 / 50 / 200 Hz, 10 dB, 200 ns, closed form next to it, and the
      same-slot single-slot estimate's for comparison;
  m   the PMI comparison, antennas = (1, 2), a PMI per 12 subcarriers: the share of subbands whose PMI chosen from the h-ahead
      prediction (W = 4) differs from the one chosen from the TRUE channel of the slot; next to it the same share for the h-slots-old
      single-slot estimate and for the h-slots-old true channel.  linksim.precoding_pmi_host on the estimates: host arithmetic.
``--device cpu`` runs sections n, h and m with the float64 twins (simulate_frames_host, lmmse_seq_estimate_host); k is skipped.
Sections n, h and m draw one-value condition tables per point, so every frame of a point is at that point.  Reported, not asserted."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lmmse_bench import _stats  # noqa: E402

LIMITS = {"k": 300, "n": 420, "h": 300, "m": 420}     # seconds per child
SLOTS = 8
WINDOWS = (1, 2, 4, 8)
DS_NS = 200.0
N_SNR, N_HZ = (0.0, 5.0, 10.0, 15.0, 20.0, 25.0, 30.0), (50.0, 200.0, 800.0)
H_SNR, H_HZ, H_WINDOW, HORIZONS = 10.0, (10.0, 50.0, 200.0), 4, (1, 2, 4)
M_SNR, M_SUBBAND, M_SEQUENCES = 15.0, 12, 320         # the set SNR and subband of profiles/link_precode_delay_bench.json
NOTE = ("device-event time per call over 200 back-to-back calls, 7 alternating rounds after 10 warm-up calls each: the allocation of the "
        "output and the launch are inside it; all variants read the same pilots and conditions")


def _point(snr, dop, **kw):
    from adafortitran_amd.chansim import ChannelSimConfig
    return ChannelSimConfig(slots=SLOTS, snr_db=(snr,), delay_spread_ns=(DS_NS,), doppler_hz=(dop,), **kw)


def _draw(a, cfg, frames, seed):
    """(ideal, pilots, meta) of `frames` frames of whole sequences: the device's simulator, or its float64 twin."""
    import numpy as np
    if a.device == "cuda":
        from adafortitran_amd.hip_ops import ChannelSimPlan
        return ChannelSimPlan(cfg, "cuda")(seed, 0, 0, 1, 1 << 40, frames)
    from adafortitran_amd.chansim import simulate_frames_host
    return simulate_frames_host(cfg, seed, np.arange(frames))


def _estimate(a, tables, pilots, meta):
    """The estimate of every frame: one launch on the device (a tensor there), or the float64 twin (a numpy array)."""
    if a.device == "cuda":
        from adafortitran_amd.hip_ops import LmmseSeqPlan
        return LmmseSeqPlan(tables, "cuda")(pilots, *(meta[:, k].contiguous() for k in range(3)))
    from adafortitran_amd.lmmse import lmmse_seq_estimate_host
    return lmmse_seq_estimate_host(tables, pilots, meta)


def _nmse_on(a, est, ideal, cfg, slots):
    """sum |est - h|^2 / sum |h|^2 over the given slots of every sequence."""
    import numpy as np
    slots = list(slots)
    if a.device == "cuda":
        import torch
        shape = (-1, cfg.slots, cfg.group * cfg.ofdm[0] * cfg.ofdm[1])
        e, h = est.reshape(shape)[:, slots], ideal.reshape(shape)[:, slots]
        return float(((e - h).abs().double() ** 2).sum() / (h.abs().double() ** 2).sum())
    shape = (-1, cfg.slots, cfg.group * cfg.ofdm[0] * cfg.ofdm[1])
    e, h = np.asarray(est).reshape(shape)[:, slots], np.asarray(ideal).reshape(shape)[:, slots]
    return float((np.abs(e - h) ** 2).sum() / (np.abs(h) ** 2).sum())


def _parent_build(path):
    """The parent commit's build with the older entry points typed from the binding's table: it lacks the new ones, so
    ``_lib.load_path`` would refuse it."""
    import ctypes
    from adafortitran_amd import _abi
    lib = ctypes.CDLL(path)
    for name in ("aft_lmmse_f32", "aft_lmmse_table_floats", "aft_last_error", "aft_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _abi.SIGNATURES[name]
    if lib.aft_version() != _abi.AFT_ABI_VERSION:
        raise SystemExit(f"{path}: ABI {lib.aft_version()}, this tree's is {_abi.AFT_ABI_VERSION}")
    return lib


def section_k(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LmmsePlan, LmmseSeqPlan
    from adafortitran_amd.lmmse import LmmseTables
    from train_loader_bench import _event_us
    cfg = ChannelSimConfig(slots=SLOTS)
    frames = a.frames - a.frames % cfg.sequence()
    _, pilots, meta = ChannelSimPlan(cfg, "cuda")(1, 0, 0, 1, 1 << 40, frames)
    conds = [meta[:, k].contiguous() for k in range(3)]
    single = LmmsePlan(cfg, "cuda")
    variants = {"aft_lmmse_f32": lambda: single(pilots, *conds)}
    plans = {W: LmmseSeqPlan(LmmseTables(cfg, W, 0), "cuda") for W in WINDOWS}
    for W, plan in plans.items():
        variants[f"aft_lmmse_seq_f32_w{W}"] = lambda p=plan: p(pilots, *conds)
    out = {"frames": frames, "slots": SLOTS, "note": NOTE}
    same = lambda x, y: bool(torch.equal(torch.view_as_real(x).view(torch.int32), torch.view_as_real(y).view(torch.int32)))  # noqa: E731
    out["w1_bits_equal_aft_lmmse_f32"] = same(plans[1](pilots, *conds), single(pilots, *conds))
    if a.parent:
        parent = _parent_build(os.path.abspath(a.parent))
        variants["aft_lmmse_f32_parent_build"] = lambda: single(pilots, *conds, lib=parent)
        out["parent"] = {"parent": os.path.basename(a.parent), "bits_equal": same(single(pilots, *conds), single(pilots, *conds, lib=parent))}
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(7):
        for k, fn in variants.items():
            us[k].append(_event_us(fn, 200))
    out.update({k: _stats(v, "us") for k, v in us.items()})
    base = out["aft_lmmse_f32"]["median_us"]
    for W in WINDOWS:
        out[f"aft_lmmse_seq_f32_w{W}"]["ratio_to_aft_lmmse_f32"] = round(out[f"aft_lmmse_seq_f32_w{W}"]["median_us"] / base, 4)
    if a.parent:
        out["parent"]["ratio_this_build_to_parent"] = round(base / out["aft_lmmse_f32_parent_build"]["median_us"], 4)
    return out


def section_n(a):
    from adafortitran_amd.lmmse import LmmseTables, lmmse_predicted_mse
    rows = []
    for dop in N_HZ:
        for snr in N_SNR:
            cfg = _point(snr, dop)
            frames = a.frames - a.frames % cfg.sequence()
            ideal, pilots, meta = _draw(a, cfg, frames, 100 + int(snr) + int(dop))
            row = {"doppler_hz": dop, "snr_db": snr, "sequences": frames // cfg.sequence()}
            for W in WINDOWS:
                tb = LmmseTables(cfg, W, 0)
                est = _estimate(a, tb, pilots, meta)
                row[f"w{W}"] = {"nmse": float(f"{_nmse_on(a, est, ideal, cfg, range(W - 1, SLOTS)):.5e}"), "steady_slots": SLOTS - W + 1,
                                "closed_form": float(f"{lmmse_predicted_mse(tb, snr, DS_NS, dop):.5e}")}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    return {"delay_spread_ns": DS_NS, "slots": SLOTS, "slot_symbols": 14, "rows": rows}


def section_h(a):
    from adafortitran_amd.lmmse import LmmseTables, lmmse_predicted_mse
    rows = []
    for dop in H_HZ:
        cfg = _point(H_SNR, dop)
        frames = a.frames - a.frames % cfg.sequence()
        ideal, pilots, meta = _draw(a, cfg, frames, 200 + int(dop))
        one = LmmseTables(cfg, 1, 0)
        row = {"doppler_hz": dop, "sequences": frames // cfg.sequence(),
               "same_slot_w1": {"nmse": float(f"{_nmse_on(a, _estimate(a, one, pilots, meta), ideal, cfg, range(SLOTS)):.5e}"),
                                "closed_form": float(f"{lmmse_predicted_mse(one, H_SNR, DS_NS, dop):.5e}")}}
        for h in (0, *HORIZONS):
            tb = LmmseTables(cfg, H_WINDOW, h)
            est = _estimate(a, tb, pilots, meta)
            steady = range(H_WINDOW - 1 + h, SLOTS)
            row[f"w{H_WINDOW}_h{h}"] = {"nmse": float(f"{_nmse_on(a, est, ideal, cfg, steady):.5e}"), "steady_slots": len(steady),
                                        "closed_form": float(f"{lmmse_predicted_mse(tb, H_SNR, DS_NS, dop):.5e}")}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"snr_db": H_SNR, "delay_spread_ns": DS_NS, "slots": SLOTS, "window": H_WINDOW, "rows": rows}


def section_m(a):
    import numpy as np
    from adafortitran_amd.linksim import LinkConfig, precoding_pmi_host, precoding_weights
    from adafortitran_amd.lmmse import LmmseTables
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)  # noqa: E731
    rows = []
    for dop in H_HZ:
        cfg = _point(M_SNR, dop, antennas=(1, 2))
        link = LinkConfig(cfg, 4)
        frames = a.sequences * cfg.sequence()
        ideal, pilots, meta = _draw(a, cfg, frames, 300 + int(dop))
        rho, _ = precoding_weights(np.full(frames, M_SNR), 0.0, 1)
        pmi = lambda est: precoding_pmi_host(link, host(est), rho, 1, M_SUBBAND).reshape(a.sequences, SLOTS, -1)  # noqa: E731
        true, single = pmi(ideal), pmi(_estimate(a, LmmseTables(cfg, 1, 0), pilots, meta))
        row = {"doppler_hz": dop, "sequences": a.sequences, "subbands": int(true.shape[-1])}
        for h in HORIZONS:
            ks = np.arange(H_WINDOW - 1 + h, SLOTS)                 # the slots with a full window: the same slots for every column
            predicted = pmi(_estimate(a, LmmseTables(cfg, H_WINDOW, h), pilots, meta))
            share = lambda got: round(float((got != true[:, ks]).mean()), 5)  # noqa: E731
            row[f"h{h}"] = {"slots_compared": len(ks), "predicted_w4": share(predicted[:, ks]), "old_single_slot_estimate": share(single[:, ks - h]),
                            "old_true_channel": share(true[:, ks - h])}
        row["same_slot_single_slot_estimate"] = round(float((single != true).mean()), 5)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"set_snr_db": M_SNR, "delay_spread_ns": DS_NS, "subband": M_SUBBAND, "antennas": [1, 2], "slots": SLOTS, "window": H_WINDOW,
            "what": "share of subbands whose PMI differs from the one chosen from the true channel of the slot", "rows": rows}


SECTIONS = {"k": section_k, "n": section_n, "h": section_h, "m": section_m}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmmse_seq_bench.json"))
    ap.add_argument("--sections", default="k,n,h,m")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--sequences", type=int, default=M_SEQUENCES, help="section m: sequences per Doppler")
    ap.add_argument("--parent", default="", help="section k: a parent build of the library to run aft_lmmse_f32 against")
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        if a.device == "cuda":
            import torch
            if not torch.cuda.is_available():
                print("lmmse_seq_bench.py: no GPU; nothing is timed without one (--device cpu runs the float64 twins)", file=sys.stderr)
                return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/lmmse_seq_bench.py", "grid": [120, 14], "pilots": [12, 2], "device": a.device, "frames": a.frames}
    status = 0
    for name in a.sections.split(","):
        if name == "k" and a.device == "cpu":
            record["k"] = "not measured: kernel times need the GPU"
            continue
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name, "--frames", str(a.frames),
               "--sequences", str(a.sequences), "--device", a.device] + (["--parent", a.parent] if a.parent else [])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"lmmse_seq_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
