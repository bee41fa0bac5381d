#!/usr/bin/env python3
"""What the HARQ link evaluation (linksim, aft_link_harq_f32) costs on one MI355X, and what it measures.

    python tools/link_harq_bench.py [--out profiles/link_harq_bench.json] [--sections k,p,s] [--frames 128] [--parent LIB]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   aft_link_harq_f32 at 128 default-grid frames of 16-QAM, mother code 1/2, as device-event time over many back-to-back launches
      in alternating rounds with aft_link_ldpc_f32 on the SAME tensors: one round of the whole codeword (Q = 1, C = nb: the same
      work as the single-shot kernel plus the soft buffer), and Q = 2 and Q = 4 rounds of 16 of the 24 columns, incremental
      redundancy and chase combining.  Beside each figure: groups, blocks per group, waves per workgroup, mean attempts and
      iterations per block;
  p   aft_link_ldpc_f32 of this build against the same entry point of another build of the library (``--parent``: the library of
      the commit before the decoder moved into csrc/linkldpc_device.h), interleaved on the same tensors; skipped without --parent;
  s   throughput (delivered information bits per data element sent), mean transmissions per block and residual block-error rate
      over the simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames: perfect channel
      knowledge, the LMMSE estimate (on the device) and the interpolated LS estimate; incremental redundancy and chase combining
      (16 of 24 columns, 4 rounds) beside the single-shot mother code.  Reported, not asserted."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from link_ldpc_bench import BATCH, NOTE, _measure, _tensors  # noqa: E402

LIMITS = {"k": 240, "p": 180, "s": 420}     # seconds per child
M, RATE, TX_COLS = 4, "1/2", 16


def _waves(harq):
    per_wave = 4 * harq.code.coded_bits + 64 * harq.code.edges                   # csrc/k_linkharq.hip link_harq_waves
    return min(16, harq.blocks, max(1, (150 * 1024) // per_wave))


def _llr(cases=((M, RATE),)):
    """``[(LdpcConfig, llr)]`` for the (bits per symbol, rate) ``cases`` on one set of frames, and the frames' keys."""
    from adafortitran_amd.hip_ops import LinkSoftPlan
    from adafortitran_amd.linksim import LdpcConfig, LinkConfig
    cfg, ideal, est, keys, sigma, scale, one = _tensors()
    out = []
    for m, rate in cases:
        link = LinkConfig(cfg, m)
        out.append((LdpcConfig(link, rate), LinkSoftPlan(link, "cuda")(ideal, est, keys, sigma, scale, one, want_llr=True)[1]))
    return out, keys


def section_k(a):
    from adafortitran_amd.hip_ops import LinkHarqPlan, LinkLdpcPlan
    from adafortitran_amd.linksim import HarqConfig
    ((code, llr),), keys = _llr()
    single = LinkLdpcPlan(code, "cuda")
    variants, shape = {"ldpc_single_shot": lambda: single(llr, keys)}, {}
    counts = single(llr, keys)[0].sum(dim=0).tolist()
    single_shape = {"blocks_per_frame": code.blocks, "bler": round(counts[1] / (BATCH * code.blocks), 4),
                    "mean_iterations": round(counts[2] / (BATCH * code.blocks), 3)}
    for name, harq in (("harq_q1_whole", HarqConfig(code, code.base_cols, 1, stride=code.stride)),
                       ("harq_q2_ir", HarqConfig(code, TX_COLS, 2)), ("harq_q4_ir", HarqConfig(code, TX_COLS, 4)),
                       ("harq_q4_chase", HarqConfig(code, TX_COLS, 4, mode="chase"))):
        plan = LinkHarqPlan(harq, "cuda")
        variants[name] = lambda p=plan: p(llr, keys)
        c = plan(llr, keys)[0].sum(dim=0).tolist()
        blocks = (BATCH // harq.rounds) * harq.blocks
        attempts = sum((t + 1) * c[t] for t in range(4)) + harq.rounds * c[5]
        shape[name] = {"groups": BATCH // harq.rounds, "blocks_per_group": harq.blocks, "waves_per_workgroup": _waves(harq),
                       "tx_cols": harq.tx_cols, "starts": list(harq.starts), "residual_bler": round(c[5] / blocks, 4),
                       "mean_attempts": round(attempts / blocks, 3), "mean_iterations": round(c[6] / blocks, 3)}
    out = _measure(variants)
    out["ldpc_single_shot"].update(single_shape)
    for name, s in shape.items():
        out[name].update(s, ldpc_single_shot_median_us=out["ldpc_single_shot"]["median_us"])
    out["case"], out["batch"], out["note"] = f"m{M}_r12", BATCH, NOTE
    return out


def _other_build(path):
    """Another build of the library, typed from the binding's table where it exports the name: a build from before
    aft_link_harq_f32 lacks it, which ``_lib.load_path`` refuses."""
    import ctypes
    from adafortitran_amd import _abi
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _abi.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    if lib.aft_version() != _abi.AFT_ABI_VERSION:
        raise SystemExit(f"{path}: ABI {lib.aft_version()}, the binding's is {_abi.AFT_ABI_VERSION}")
    return lib


def section_p(a):
    from adafortitran_amd.hip_ops import LinkLdpcPlan
    import torch
    made, keys = _llr(((M, RATE), (8, (3, 4))))                                  # 4 blocks per frame, and 51: more blocks than waves
    parent = _other_build(os.path.abspath(a.parent))
    variants, same = {}, {}
    cases = dict(zip((f"m{M}_r12", "m8_r3x4"), made))
    for name, (c, t) in cases.items():
        plan = LinkLdpcPlan(c, "cuda")
        variants[f"{name}_this_build"] = lambda p=plan, t=t: p(t, keys)
        variants[f"{name}_parent_build"] = lambda p=plan, t=t: p(t, keys, lib=parent)
        here, there = plan(t, keys, want_bits=True), plan(t, keys, want_bits=True, lib=parent)
        same[name] = bool(torch.equal(here[0], there[0]) and torch.equal(here[1], there[1]))
    # twice, the second time with the two builds of a case in the other order inside a round: what follows what is not the build's
    orders = {"this_build_first": _measure(variants), "parent_build_first": _measure(dict(reversed(list(variants.items()))))}
    out = dict(orders)
    for name in cases:
        this = [o[f"{name}_this_build"] for o in orders.values()]
        par = [o[f"{name}_parent_build"] for o in orders.values()]
        lo, hi = min(p["min_us"] for p in par), max(p["max_us"] for p in par)
        medians = [t["median_us"] for t in this]
        out[name] = {"outputs_identical": same[name],
                     "median_difference_us": [round(t["median_us"] - p["median_us"], 4) for t, p in zip(this, par)],
                     "parent_range_us": [lo, hi], "parent_spread_us": round(hi - lo, 4),
                     "within_the_parents_spread": bool(all(m <= hi for m in medians))}
    out["batch"], out["note"] = BATCH, NOTE
    return out


def section_s(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import HarqAccumulator, HarqConfig, LdpcBlockErrorAccumulator, LdpcConfig, LinkConfig
    from adafortitran_amd.lmmse import LmmseEstimator
    cfg = ChannelSimConfig()
    model = LmmseEstimator(cfg).to("cuda")
    ds, dop = 200.0, 800.0
    sc, sym = np.asarray(cfg.pilot_scs), np.asarray(cfg.pilot_symbols)
    code = LdpcConfig(LinkConfig(cfg, M), RATE)
    schemes = {"ir": HarqConfig(code, TX_COLS, 4), "chase": HarqConfig(code, TX_COLS, 4, mode="chase"), "single_shot": code}
    rows = []
    for snr in cfg.snr_db:
        pack = make_pack(cfg, a.frames, seed=100 + int(snr), snr_db=snr, delay_spread_ns=ds, doppler_hz=dop)
        ideal, ls = torch.from_numpy(pack["h_ideal"]).cuda(), torch.from_numpy(pack["h_ls_full"]).cuda()
        pilots = torch.from_numpy(np.ascontiguousarray(pack["h_ls_sparse"][:, sc[:, None], sym[None, :]])).cuda()
        meta = torch.from_numpy(pack["meta"])
        accs = {(s, which): (HarqAccumulator if isinstance(c, HarqConfig) else LdpcBlockErrorAccumulator)(c, "cuda", seed=1)
                for s, c in schemes.items() for which in ("perfect", "lmmse", "ls")}
        for lo in range(0, a.frames, BATCH):
            sl = slice(lo, lo + BATCH)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (s, which), acc in accs.items():
                acc.update(est[which], ideal[sl], cols)
        row = {"snr_db": int(snr)}
        for (s, which), acc in accs.items():
            cell = {"throughput": round(acc.result_throughput(), 4), "residual_bler": round(acc.result(), 4)}
            if s != "single_shot":
                cell["transmissions"] = round(acc.result_transmissions(), 3)
            row[f"{s}_{which}"] = cell
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"frames_per_set": a.frames, "delay_spread_ns": ds, "doppler_hz": dop, "case": f"m{M}_r12", "tx_cols": TX_COLS, "rounds": 4,
            "blocks_per_round_frame": schemes["ir"].blocks, "blocks_per_frame_single_shot": code.blocks, "rows": rows}


SECTIONS = {"k": section_k, "p": section_p, "s": section_s}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_harq_bench.json"))
    ap.add_argument("--sections", default="k,p,s")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--parent", default="", help="another build of the library for section p")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.frames % (4 * 2) or a.frames % BATCH:
        ap.error(f"--frames must be a multiple of {BATCH}")
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("link_harq_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_harq_bench.py", "grid": [120, 14], "pilots": [12, 2]}
    status = 0
    for name in a.sections.split(","):
        if name == "p" and not a.parent:
            record["p"] = "skipped: no --parent library given"
            continue
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames), "--parent", a.parent]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_harq_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
