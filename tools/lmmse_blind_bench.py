#!/usr/bin/env python3
"""What choosing the LMMSE design point from the pilots (lmmse.ConditionEstimator, aft_lmmse_classify_f32) costs on one MI355X, how
often it is right, and what the blind estimator loses against the genie-aided one.

    python tools/lmmse_blind_bench.py [--out profiles/lmmse_blind_bench.json] [--sections k,r,a] [--frames 4096] [--parent LIB]
                                      [--device cuda|cpu]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the classify kernel at W = 1, 2, 4, 8 and G = 1, 4 on `--frames` frames of the default grid in sequences of K = 8 slots, next to
      aft_lmmse_seq_f32 on the same pilots: device-event time per call over back-to-back calls, in alternating rounds (the warm-up and
      repeat rules of tools/lmmse_bench.py).  With ``--parent LIB`` aft_lmmse_f32 and aft_lmmse_seq_f32 (W = 4) of that build run in
      the same rounds and their bits are compared with this build's.  Needs a GPU;
  r   per configuration (slots = 1; slots = 8 with W = 4 and W = 8; slots = 8, W = 4, antennas = (4, 1) pooled over the group), default
      grids, all conditions, steady slots: hit rate and within-one-bin rate per condition, overall, per true SNR and per true Doppler;
      NMSE genie (the simulator's meta) / blind (the maximum-likelihood pick) / robust (``assume`` at the grid's highest SNR, delay
      spread and Doppler);
  a   AdaFortiTran with given and with estimated condition tokens (lmmse.EstimatedConditions, measured by get_test_stats), after the
      short training of tools/synth_loader_bench.py (300 steps, seed 7) or on a pickled module given with ``--checkpoint``; the
      LMMSE baseline both ways beside it.  Needs a GPU;
``--device cpu`` runs section r with the float64 twins (simulate_frames_host, lmmse_classify_host, lmmse_seq_estimate_host); k and a
say that they need the GPU.  Reported, not asserted."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lmmse_bench import _stats  # noqa: E402

LIMITS = {"k": 420, "r": 420, "a": 300}     # seconds per child
SLOTS = 8
WINDOWS = (1, 2, 4, 8)
GROUPS = (1, 4)
NOTE = ("device-event time per call over 100 back-to-back calls, 6 alternating rounds (every other one in reverse order) after 5 warm-up "
        "calls each: the allocation of the outputs and the launch are inside it; classify and estimate read the same pilots")
# name: (slots, antennas, W, sequences per 4096 frames are derived)
R_CONFIGS = {"slots1": (1, (1, 1), 1), "slots8_w4": (8, (1, 1), 4), "slots8_w8": (8, (1, 1), 8), "slots8_w4_antennas4x1_pooled": (8, (4, 1), 4)}


def _parent_build(path):
    """The parent commit's build with the older entry points typed from the binding's table: it lacks the new ones, so
    ``_lib.load_path`` would refuse it."""
    import ctypes
    from adafortitran_amd import _abi
    lib = ctypes.CDLL(path)
    for name in ("aft_lmmse_f32", "aft_lmmse_table_floats", "aft_lmmse_seq_f32", "aft_lmmse_seq_table_floats", "aft_last_error", "aft_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _abi.SIGNATURES[name]
    if lib.aft_version() != _abi.AFT_ABI_VERSION:
        raise SystemExit(f"{path}: ABI {lib.aft_version()}, this tree's is {_abi.AFT_ABI_VERSION}")
    return lib


def section_k(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LmmseClassifyPlan, LmmsePlan, LmmseSeqPlan
    from adafortitran_amd.lmmse import LmmseTables
    from train_loader_bench import _event_us
    out = {"slots": SLOTS, "note": NOTE}
    variants, keep = {}, []
    for G in GROUPS:
        cfg = ChannelSimConfig(slots=SLOTS, antennas=(G, 1))
        frames = a.frames - a.frames % cfg.sequence()
        _, pilots, meta = ChannelSimPlan(cfg, "cuda")(1, 0, 0, 1, 1 << 40, frames)
        conds = [meta[:, k].contiguous() for k in range(3)]
        keep.append((pilots, conds))
        out[f"frames_g{G}"] = frames
        for W in WINDOWS:
            tb = LmmseTables(cfg, W, 0)
            seq, cl = LmmseSeqPlan(tb, "cuda"), LmmseClassifyPlan(tb, "cuda")
            variants[f"aft_lmmse_seq_f32_w{W}_g{G}"] = lambda p=seq, x=pilots, c=conds: p(x, *c)
            variants[f"aft_lmmse_classify_f32_w{W}_g{G}"] = lambda p=cl, x=pilots: p(x)
            if G == 1 and W == 4:
                variants["aft_lmmse_classify_f32_w4_g1_with_scores"] = lambda p=cl, x=pilots: p(x, scores=True)
    if a.parent:
        parent = _parent_build(os.path.abspath(a.parent))
        pilots, conds = keep[0]
        cfg = ChannelSimConfig(slots=SLOTS)
        single, seq4 = LmmsePlan(cfg, "cuda"), LmmseSeqPlan(LmmseTables(cfg, 4, 0), "cuda")
        same = lambda x, y: bool(torch.equal(torch.view_as_real(x).view(torch.int32), torch.view_as_real(y).view(torch.int32)))  # noqa: E731
        out["parent"] = {"parent": os.path.basename(a.parent),
                         "aft_lmmse_f32_bits_equal": same(single(pilots, *conds), single(pilots, *conds, lib=parent)),
                         "aft_lmmse_seq_f32_w4_bits_equal": same(seq4(pilots, *conds), seq4(pilots, *conds, lib=parent))}
        variants["aft_lmmse_f32"] = lambda: single(pilots, *conds)
        variants["aft_lmmse_f32_parent_build"] = lambda: single(pilots, *conds, lib=parent)
        variants["aft_lmmse_seq_f32_w4_g1_parent_build"] = lambda: seq4(pilots, *conds, lib=parent)
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    order = list(variants.items())
    for r in range(6):                       # every other round backwards: what a variant inherits from the one before it cancels
        for k, fn in (order if r % 2 == 0 else reversed(order)):
            us[k].append(_event_us(fn, 100))
    out.update({k: _stats(v, "us") for k, v in us.items()})
    for G in GROUPS:
        for W in WINDOWS:
            out[f"aft_lmmse_classify_f32_w{W}_g{G}"]["ratio_to_aft_lmmse_seq_f32"] = round(
                out[f"aft_lmmse_classify_f32_w{W}_g{G}"]["median_us"] / out[f"aft_lmmse_seq_f32_w{W}_g{G}"]["median_us"], 4)
    if a.parent:
        out["parent"]["aft_lmmse_f32_ratio_this_build_to_parent"] = round(out["aft_lmmse_f32"]["median_us"] / out["aft_lmmse_f32_parent_build"]["median_us"], 4)
        out["parent"]["aft_lmmse_seq_f32_w4_ratio_this_build_to_parent"] = round(
            out["aft_lmmse_seq_f32_w4_g1"]["median_us"] / out["aft_lmmse_seq_f32_w4_g1_parent_build"]["median_us"], 4)
    return out


def _rates(true, got, by):
    """Hit and within-one-bin rate of index arrays, overall and per value of ``by``."""
    import numpy as np
    hit, near = true == got, np.abs(true - got) <= 1
    return {"hit": round(float(hit.mean()), 4), "within_one": round(float(near.mean()), 4),
            "per": {int(v): [round(float(hit[by == v].mean()), 4), round(float(near[by == v].mean()), 4)] for v in np.unique(by)}}


def section_r(a):
    import numpy as np
    from adafortitran_amd.chansim import ChannelSimConfig, simulate_frames_host
    from adafortitran_amd.lmmse import CONDITIONS, LmmseTables, lmmse_classify_host, lmmse_estimate_host, lmmse_seq_estimate_host
    out = {"what": "steady slots, all conditions of the default grids; per: {true index: [hit, within one bin]}"}
    for name, (slots, antennas, W) in R_CONFIGS.items():
        cfg = ChannelSimConfig(slots=slots, antennas=antennas)
        frames = a.frames - a.frames % cfg.sequence()
        tb = LmmseTables(cfg, W, 0)
        top = {k: float(tb.values[k].max()) for k in CONDITIONS}
        if a.device == "cuda":
            import torch
            from adafortitran_amd.hip_ops import ChannelSimPlan, LmmseClassifyPlan, LmmsePlan, LmmseSeqPlan
            ideal, pilots, meta = ChannelSimPlan(cfg, "cuda")(7, 0, 0, 1, 1 << 40, frames)
            idx, snr, ds, dop = LmmseClassifyPlan(tb, "cuda")(pilots)
            plan = LmmseSeqPlan if tb.multi_slot else LmmsePlan
            conds = [meta[:, k].contiguous() for k in range(3)]
            ests = [plan(tb, "cuda")(pilots, *conds), plan(tb, "cuda")(pilots, snr, ds, dop), plan(tb, "cuda", assume=top)(pilots)]
            torch.cuda.synchronize()
            ideal, meta, idx = ideal.cpu().numpy(), meta.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
            ests = [e.cpu().numpy() for e in ests]
        else:
            ideal, pilots, meta = simulate_frames_host(cfg, 7, np.arange(frames))
            idx, values = lmmse_classify_host(tb, pilots)
            host = lmmse_seq_estimate_host if tb.multi_slot else lmmse_estimate_host
            ests = [host(tb, pilots, meta), host(tb, pilots, values), host(tb, pilots, None, top)]
        steady = np.arange(frames) // cfg.group % cfg.slots >= W - 1
        true = np.stack(tb.indices(meta), axis=1)
        nmse = lambda e: float(f"{(np.abs(e - ideal)[steady] ** 2).sum() / (np.abs(ideal)[steady] ** 2).sum():.5e}")  # noqa: E731
        row = {"slots": slots, "antennas": list(antennas), "window": W, "frames": frames, "steady_frames": int(steady.sum()),
               "nmse_genie": nmse(ests[0]), "nmse_blind": nmse(ests[1]), "nmse_robust": nmse(ests[2]), "robust_assume": top}
        for k, cond in enumerate(CONDITIONS):
            row[cond] = {"by_true_snr": _rates(true[steady, k], idx[steady, k], true[steady, 0]),
                         "by_true_doppler": _rates(true[steady, k], idx[steady, k], true[steady, 2])}
        out[name] = row
        print(json.dumps({k: row[k] for k in ("nmse_genie", "nmse_blind", "nmse_robust")} | {"config": name} |
                         {c: [row[c]["by_true_snr"]["hit"], row[c]["by_true_snr"]["within_one"]] for c in CONDITIONS}), file=sys.stderr)
    return out


def section_a(a):
    """AdaFortiTran after the short training of tools/synth_loader_bench.py (section t: the default model, dropout 0, ShardedFlatAdam,
    batches of 128 simulated frames, seed 7), or a pickled module given with --checkpoint: MSE in dB per SNR with the loader's
    condition tokens and with the tokens estimated from the pilots, and the LMMSE baseline both ways on the same frames."""
    if a.device != "cuda":
        return {"measured": False, "why": "the short training runs on the HIP device: --device cuda"}
    import torch
    import train_bench
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, make_pack
    from adafortitran_amd.evaluation import get_test_stats
    from adafortitran_amd.lmmse import EstimatedConditions, LmmseEstimator
    from adafortitran_amd.optim import ShardedFlatAdam
    cfg = ChannelSimConfig()
    out = {"measured": True, "what": "MSE in dB per SNR over 512 simulated frames each (all delay spreads and Dopplers of the default grids)"}
    if a.checkpoint:
        model = torch.load(a.checkpoint, weights_only=False).to("cuda")
        out["model"] = {"checkpoint": os.path.basename(a.checkpoint)}
    else:
        torch.manual_seed(0)
        model = train_bench.build("adafortitran", 0.0).train()
        opt = ShardedFlatAdam(model.parameters(), lr=a.lr)
        losses = []
        for pilots, ideal, meta in SynthLoader(cfg, 128, 128 * a.train_steps, device="cuda", seed=7):
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(torch.view_as_real(model(pilots, meta)), torch.view_as_real(ideal))
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        losses = torch.stack(losses).cpu().numpy()
        win = max(1, a.train_steps // 12)
        out["model"] = {"training": "tools/synth_loader_bench.py section t", "seed": 7, "batch": 128, "steps": int(len(losses)), "lr": a.lr,
                        "dropout": 0.0, "first_loss": round(float(losses[:win].mean()), 6), "final_loss": round(float(losses[-win:].mean()), 6)}
    model = model.eval()
    packs = {snr: make_pack(cfg, 512, seed=40 + snr, snr_db=snr) for snr in (0, 10, 20, 30)}
    loaders = lambda: [(f"SNR_{snr}", ingest.ResidentLoader(p, cfg.pilot, 128, device="cuda", shuffle=False)) for snr, p in packs.items()]  # noqa: E731
    rnd = lambda st: {k: round(v, 4) for k, v in st.items()}  # noqa: E731
    with torch.no_grad():
        out["adafortitran_given_tokens"] = rnd(get_test_stats(model, loaders()))
        out["adafortitran_estimated_tokens"] = rnd(get_test_stats(EstimatedConditions(model, cfg).to("cuda"), loaders()))
        out["lmmse_given_conditions"] = rnd(get_test_stats(LmmseEstimator(cfg).to("cuda"), loaders()))
        out["lmmse_estimated_conditions"] = rnd(get_test_stats(LmmseEstimator(cfg, conditions="estimated").to("cuda"), loaders()))
    out["loss_db_from_estimating_tokens"] = {k: round(out["adafortitran_estimated_tokens"][k] - out["adafortitran_given_tokens"][k], 4)
                                             for k in out["adafortitran_given_tokens"]}
    return out


SECTIONS = {"k": section_k, "r": section_r, "a": section_a}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmmse_blind_bench.json"))
    ap.add_argument("--sections", default="k,r,a")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--parent", default="", help="section k: a parent build of the library to run the existing LMMSE kernels against")
    ap.add_argument("--checkpoint", default="", help="section a: a pickled AdaFortiTranEstimator to measure in place of the short training")
    ap.add_argument("--train-steps", type=int, default=300, help="section a: steps of the short training")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        if a.device == "cuda":
            import torch
            if not torch.cuda.is_available():
                print("lmmse_blind_bench.py: no GPU; nothing is timed without one (--device cpu runs the float64 twins)", file=sys.stderr)
                return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/lmmse_blind_bench.py", "grid": [120, 14], "pilots": [12, 2], "device": a.device, "frames": a.frames}
    status = 0
    for name in a.sections.split(","):
        if name == "k" and a.device == "cpu":
            record["k"] = "not measured: kernel times need the GPU"
            continue
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name, "--frames", str(a.frames),
               "--device", a.device, "--train-steps", str(a.train_steps), "--lr", str(a.lr)] + (["--parent", a.parent] if a.parent else []) + (["--checkpoint", a.checkpoint] if a.checkpoint else [])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"lmmse_blind_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
