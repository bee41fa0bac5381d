#!/usr/bin/env python3
"""What decision-directed refinement (linksim.DataAidedRefiner: aft_link_observe_f32, then aft_lmmse_grid_f32) costs on one MI355X and
what it buys or loses per SNR.

    python tools/link_dd_bench.py [--out profiles/link_dd_bench.json] [--sections k,r,a] [--frames 4096] [--parent LIB]
                                  [--device cuda|cpu]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   the two kernels on `--frames` frames of the default grid, 16-QAM, beside aft_lmmse_f32 (the pilot estimator on the same frames'
      pilots) and aft_link_soft_f32 / aft_link_mrc_f32 (the link kernels on the same tensors, R = 1 and R = 2): device-event time per
      call over back-to-back calls in alternating rounds (the warm-up and repeat rules of tools/lmmse_bench.py), and the achieved
      bytes per second against the ALGORITHMIC bytes -- what a call must move at least: observe reads H and E and writes z (24 S T
      bytes per frame) and a byte per element and group; the smoother reads z and writes est (16 S T per frame).  With ``--parent
      LIB`` aft_lmmse_f32 and aft_lmmse_seq_f32 (W = 4) of that build run in the same rounds and their bits are compared with this
      build's (the pilot kernels share their second half with the smoother now).  Needs a GPU;
  r   per SNR (0 .. 30 dB, all delay spreads and Dopplers), QPSK and 16-QAM: NMSE, BER and LDPC BLER (rate 1/2) of the LMMSE and the
      LS-interpolated estimate after 0, 1 and 2 passes, and the NMSE with the sent symbols known (the genie bound);
  a   the same for an AdaFortiTran after the short training of tools/synth_loader_bench.py (300 steps, seed 7) or a pickled module given
      with ``--checkpoint``.  Needs a GPU;
``--device cpu`` runs section r with the float64 twins on fewer frames; k and a say that they need the GPU.  Reported, not asserted:
nobody had measured these kernels, and where refinement HURTS (low SNR: most decisions are wrong) the table says so."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lmmse_bench import _stats  # noqa: E402
from lmmse_blind_bench import _parent_build  # noqa: E402

LIMITS = {"k": 420, "r": 540, "a": 420}     # seconds per child
SNRS = (0, 10, 20, 30)
NOTE = ("device-event time per call over 100 back-to-back calls, 6 alternating rounds (every other one in reverse order) after 5 warm-up "
        "calls each: the allocation of the outputs and the launch are inside it; every variant reads the same tensors")


def section_k(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import (ChannelSimPlan, LinkMrcPlan, LinkObservePlan, LinkSoftPlan, LmmseGridPlan, LmmsePlan,
                                          LmmseSeqPlan)
    from adafortitran_amd.linksim import LinkConfig, data_noise_scale, frame_keys_torch
    from adafortitran_amd.lmmse import LmmseTables
    from train_loader_bench import _event_us
    sim, m = ChannelSimConfig(), 4
    cfg, tb = LinkConfig(sim, m), LmmseTables(sim)
    S, T = sim.ofdm
    n = a.frames - a.frames % 2
    ideal, pilots, meta = ChannelSimPlan(sim, "cuda")(1, 0, 0, 1, 1 << 40, n)
    conds = [meta[:, k].contiguous() for k in range(3)]
    keys = frame_keys_torch(1, torch.arange(n, device="cuda"))
    sigma = torch.pow(10.0, -conds[0].double() / 20.0).float()
    scale = (1.0 / torch.pow(10.0, -conds[0].double() / 10.0)).float()
    rho1 = torch.ones(n, device="cuda")
    rho2 = (scale.view(-1, 2).double() / scale.view(-1, 2)[:, :1].double()).float().reshape(-1)
    one = torch.ones(1, device="cuda")
    pilot = LmmsePlan(tb, "cuda")
    est = pilot(pilots, *conds)
    obs1, obs2 = LinkObservePlan(cfg, "cuda", 1), LinkObservePlan(cfg, "cuda", 2)
    grid = LmmseGridPlan(tb, "cuda", noise_scale=data_noise_scale(m))
    soft, mrc2 = LinkSoftPlan(cfg, "cuda"), LinkMrcPlan(cfg, "cuda", 2)
    z = obs1(ideal, est, keys, sigma, rho1, pilots)[0]
    variants = {
        "aft_link_observe_f32_r1": lambda: obs1(ideal, est, keys, sigma, rho1, pilots),
        "aft_link_observe_f32_r2": lambda: obs2(ideal, est, keys, sigma, rho2, pilots),
        "aft_lmmse_grid_f32": lambda: grid(z, *conds),
        "aft_lmmse_f32": lambda: pilot(pilots, *conds),
        "aft_link_soft_f32": lambda: soft(ideal, est, keys, sigma, scale, one),
        "aft_link_mrc_f32_r2": lambda: mrc2(ideal, est, keys, sigma, rho2, scale[::2].contiguous(), one),
    }
    frame = 8 * S * T                      # bytes of one complex64 plane
    algorithmic = {"aft_link_observe_f32_r1": n * (3 * frame + S * T), "aft_link_observe_f32_r2": n * 3 * frame + n // 2 * S * T,
                   "aft_lmmse_grid_f32": n * 2 * frame, "aft_lmmse_f32": n * (frame + 8 * sim.pilot[0] * sim.pilot[1]),
                   "aft_link_soft_f32": n * 2 * frame, "aft_link_mrc_f32_r2": n * 2 * frame}
    out = {"frames": n, "bits_per_symbol": m, "kf": grid.kf, "note": NOTE,
           "algorithmic_bytes": "the least a call must move: the planes it reads and writes once each, tables and per-frame scalars left out"}
    if a.parent:
        parent = _parent_build(os.path.abspath(a.parent))
        seq_cfg = ChannelSimConfig(slots=8)
        ns = n - n % 8
        _, sp, smeta = ChannelSimPlan(seq_cfg, "cuda")(1, 0, 0, 1, 1 << 40, ns)
        sconds = [smeta[:, k].contiguous() for k in range(3)]
        seq4 = LmmseSeqPlan(LmmseTables(seq_cfg, 4, 0), "cuda")
        same = lambda x, y: bool(torch.equal(torch.view_as_real(x).view(torch.int32), torch.view_as_real(y).view(torch.int32)))  # noqa: E731
        out["parent"] = {"parent": os.path.basename(a.parent),
                         "aft_lmmse_f32_bits_equal": same(pilot(pilots, *conds), pilot(pilots, *conds, lib=parent)),
                         "aft_lmmse_seq_f32_w4_bits_equal": same(seq4(sp, *sconds), seq4(sp, *sconds, lib=parent))}
        variants["aft_lmmse_f32_parent_build"] = lambda: pilot(pilots, *conds, lib=parent)
        variants["aft_lmmse_seq_f32_w4"] = lambda: seq4(sp, *sconds)
        variants["aft_lmmse_seq_f32_w4_parent_build"] = lambda: seq4(sp, *sconds, lib=parent)
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
    for k, b in algorithmic.items():
        out[k]["algorithmic_bytes"] = int(b)
        out[k]["achieved_tb_per_s"] = round(b / out[k]["median_us"] * 1e-6, 3)
    out["refine_pass_us"] = round(out["aft_link_observe_f32_r1"]["median_us"] + out["aft_lmmse_grid_f32"]["median_us"], 2)
    if a.parent:
        out["parent"]["aft_lmmse_f32_ratio_this_build_to_parent"] = round(out["aft_lmmse_f32"]["median_us"] / out["aft_lmmse_f32_parent_build"]["median_us"], 4)
        out["parent"]["aft_lmmse_seq_f32_w4_ratio_this_build_to_parent"] = round(
            out["aft_lmmse_seq_f32_w4"]["median_us"] / out["aft_lmmse_seq_f32_w4_parent_build"]["median_us"], 4)
    return out


def _table(model_of, a, device, frames):
    """{model: {m: {snr: {passes: {nmse_db, ber, bler}}, genie_nmse_db}}} over packs of `frames` frames per SNR."""
    import torch
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.evaluation import get_link_bler, get_link_stats, get_refined_test_stats, get_test_stats
    from adafortitran_amd.linksim import DataAidedRefiner, LdpcConfig, LinkConfig
    sim = ChannelSimConfig()
    packs = {snr: make_pack(sim, frames, seed=40 + snr, snr_db=snr) for snr in SNRS}
    loaders = lambda: [(f"SNR_{snr}", ingest.ResidentLoader(p, sim.pilot, min(frames, 128), device=device, shuffle=False))  # noqa: E731
                       for snr, p in packs.items()]
    rnd = lambda st, k=5: {s: round(v, k) for s, v in st.items()}  # noqa: E731
    out = {}
    with torch.no_grad():
        for name, model in model_of(sim).items():
            out[name] = {}
            for m in (2, 4):
                cfg = LinkConfig(sim, m)
                code = LdpcConfig(cfg, "1/2")
                row = {}
                for passes in (0, 1, 2):
                    refine = passes or None
                    row[f"passes_{passes}"] = {
                        "nmse_db": rnd(get_test_stats(model, loaders()) if passes == 0 else
                                       get_refined_test_stats(model, loaders(), cfg, refine=passes, seed=5), 3),
                        "ber": rnd(get_link_stats(model, loaders(), cfg, seed=5, refine=refine)),
                        "ldpc_bler": rnd(get_link_bler(model, loaders(), code, seed=5, refine=refine), 4)}
                genie = DataAidedRefiner(cfg, device, 5, source="sent")
                row["genie_nmse_db"] = rnd(get_refined_test_stats(model, loaders(), cfg, refine=genie, seed=5), 3)
                row["refinement_hurts_nmse_at_snr"] = [s for s in SNRS if row["passes_1"]["nmse_db"][s] > row["passes_0"]["nmse_db"][s]]
                out[name][f"m{m}"] = row
    return out


def _ls_model(sim, device):
    import torch
    from adafortitran_amd.chansim import ls_interpolate

    class Ls(torch.nn.Module):
        """The LS-interpolated estimate as a model ``evaluation.forward_pass`` can call (interpolated on the host)."""

        def __init__(self):
            super().__init__()
            self.register_buffer("anchor", torch.zeros(1))

        def forward(self, pilots):
            return torch.from_numpy(ls_interpolate(sim, pilots.cpu().numpy())).to(self.anchor.device)

    return Ls().to(device)


def section_r(a):
    from adafortitran_amd.lmmse import LmmseEstimator
    frames = 512 if a.device == "cuda" else 64
    out = {"what": f"{frames} simulated frames per SNR (all delay spreads and Dopplers of the default grids); NMSE in dB, bit-error rate, "
                   f"LDPC rate-1/2 block-error rate after 0 / 1 / 2 decision-directed passes; genie: one pass with the sent symbols known",
           "frames_per_snr": frames}
    out.update(_table(lambda sim: {"lmmse": LmmseEstimator(sim).to(a.device), "ls": _ls_model(sim, a.device)}, a, a.device, frames))
    return out


def section_a(a):
    if a.device != "cuda":
        return {"measured": False, "why": "the short training runs on the HIP device: --device cuda"}
    import torch
    import train_bench
    from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader
    from adafortitran_amd.optim import ShardedFlatAdam
    out = {"measured": True}
    if a.checkpoint:
        model = torch.load(a.checkpoint, weights_only=False).to("cuda")
        out["model"] = {"checkpoint": os.path.basename(a.checkpoint)}
    else:
        torch.manual_seed(0)
        model = train_bench.build("adafortitran", 0.0).train()
        opt = ShardedFlatAdam(model.parameters(), lr=a.lr)
        losses = []
        for pilots, ideal, meta in SynthLoader(ChannelSimConfig(), 128, 128 * a.train_steps, device="cuda", seed=7):
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
    out.update(_table(lambda sim: {"adafortitran": model}, a, "cuda", 512))
    return out


SECTIONS = {"k": section_k, "r": section_r, "a": section_a}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_dd_bench.json"))
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
                print("link_dd_bench.py: no GPU; nothing is timed without one (--device cpu runs the float64 twins)", file=sys.stderr)
                return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_dd_bench.py", "grid": [120, 14], "pilots": [12, 2], "device": a.device, "frames": a.frames}
    status = 0
    for name in a.sections.split(","):
        if name == "k" and a.device == "cpu":
            record["k"] = "not measured: kernel times need the GPU"
            continue
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name, "--frames", str(a.frames),
               "--device", a.device, "--train-steps", str(a.train_steps), "--lr", str(a.lr)] + (["--parent", a.parent] if a.parent else []) + \
              (["--checkpoint", a.checkpoint] if a.checkpoint else [])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_dd_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
