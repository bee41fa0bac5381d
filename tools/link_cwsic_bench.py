#!/usr/bin/env python3
"""What codeword-level cancellation on the two-stream link (linksim "the codeword-cancellation link": aft_link_cancel_f32 and
aft_link_ldpc_masked_f32 behind aft_link_sm_f32 and aft_link_ldpc_f32) costs on one MI355X, and what it measures beside the MMSE
detector, symbol-level cancellation and the joint demapper.

    python tools/link_cwsic_bench.py [--out profiles/link_cwsic_bench.json] [--sections k,d,c,b] [--frames 128] [--device cuda|cpu] [--parent LIB]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   link_cancel_kernel at m = 2, 4, 6 and 8 on 2 x 2 and 2 x 4, at one factor with its LLR and state outputs, as device-event time
      over many back-to-back launches, in alternating rounds with link_sm_kernel (aft_link_sm_f32, MMSE) on the SAME tensors in the
      same process, at G = 32 groups and at G = 256 (one workgroup per compute unit), for three ``failed`` patterns: ``none`` (no
      group is detected again: every workgroup only stores zeros), ``every`` (every group detects one stream again, alternating
      which) and ``mix`` (the block-error counts the LDPC decoder, rate 1/2, leaves for the linear kernel's LLRs of these frames,
      read in place at stride 3).  ``ratio_to_sm`` per pattern is a description, not a target.
      With ``--parent LIB`` (a build of the parent commit's library, loaded beside this one) aft_link_sm_f32 also runs on that
      library on the same operands, interleaved with this build in both orders: ``parent`` records both medians, the parent's own
      round-to-round spread, whether this build's median lies within it, and whether all outputs are equal bit for bit;
  d   link_ldpc_kernel<masked> beside link_ldpc_kernel (aft_link_ldpc_f32) on the same LLRs and keys (rate 1/2, the linear kernel's
      LLRs at m = 2 and 4, 2 x 2, G = 256: 512 stream-frames): mask all ones, the ``mix`` above (the streams the cancel kernel flags)
      and all zeros.  With ``--parent`` aft_link_ldpc_f32 against the parent's build as in section k, counts and bits compared;
  c   the four-launch batch (LdpcBlockErrorAccumulator(detector="cwsic").update) beside the two-launch MMSE batch on the same
      device-resident frames, frame numbers and SNRs: device-event time per update, at m = 2 and 4, 2 x 2, 128 frames;
  b   LDPC block-error rate (rate 1/2) before and after cancellation, throughput and ``cwsic_stats`` at QPSK and 16-QAM over the
      simulator's SNR grid at a mid delay spread and Doppler, make_pack sets of ``--frames`` frames, 2 x R with R = 2 and 4: perfect
      channel knowledge, the LMMSE estimate and the interpolated LS estimate, beside ``mmse``, ``sic`` and ``joint`` on the same
      frames.  No trained checkpoint is read: that estimator's column stays unmeasured.  Reported, not asserted.  With
      ``--device cpu`` the host twins run in place of the kernels (sections k, d and c are skipped).
Times are read from device events; no counter profile is taken."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 400, "d": 300, "c": 200, "b": 1100}     # seconds per child
GROUP_COUNTS = (32, 256)          # workgroups: a 128-frame batch at R = 2, and one per compute unit
BRANCHES = (2, 4)
KERNEL_BITS = (2, 4, 6, 8)
BLER_BITS = (2, 4)                # section b: QPSK and 16-QAM
DETECTORS = ("mmse", "sic", "joint", "cwsic")
PATTERNS = ("none", "every", "mix")

NOTE = ("device-event time per call over 100 back-to-back calls, 5 alternating rounds: the allocations of the outputs and the launch are "
        "inside it; the kernels run at one factor with their LLR output on the same 2 G R frames (LMMSE estimates, the simulator's "
        "conditions drawn per frame, so the weights are mixed), G workgroups each")


def _parent_build(path):
    """The parent commit's build with the older entry points typed from the binding's table: it lacks the new ones, so
    ``_lib.load_path`` would refuse it."""
    import ctypes
    from adafortitran_amd import _abi
    lib = ctypes.CDLL(path)
    for name in ("aft_link_sm_f32", "aft_link_ldpc_f32", "aft_last_error", "aft_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _abi.SIGNATURES[name]
    return lib


def _against_parent(mine, theirs, same):
    """Two builds of one entry point on the same operands, interleaved in both orders: this build first in one measurement, the
    parent's first in the other, five alternating rounds each."""
    from link_mrc_bench import _measure
    a, b = _measure({"this": mine, "parent": theirs}), _measure({"parent": theirs, "this": mine})
    row = {"this_first": a, "parent_first": b, "bits_equal": bool(same)}
    medians = {k: sorted((a[k]["median_us"], b[k]["median_us"])) for k in ("this", "parent")}
    spread = max(a["parent"]["spread_us"], b["parent"]["spread_us"], medians["parent"][1] - medians["parent"][0])
    row["parent_round_to_round_spread_us"] = round(spread, 4)
    row["median_difference_us"] = round(sum(medians["this"]) / 2 - sum(medians["parent"]) / 2, 4)
    row["within_parent_spread"] = bool(abs(row["median_difference_us"]) <= spread)
    return row


def _frames(G, R, m, mix_code=None):
    """The operands of both two-stream kernels on 2 G R frames and the three ``failed`` patterns, the measured one from the decoder."""
    import torch
    from adafortitran_amd.hip_ops import LinkLdpcPlan, LinkSmPlan
    from adafortitran_amd.linksim import LdpcConfig, LinkConfig
    from link_mrc_bench import _tensors
    cfg, ideal, est, keys, sigma, scale = _tensors(G * 2 * R)
    s = scale.view(G, 2 * R).double()
    rho, lead = (s / s[:, :1]).float().reshape(-1), scale[::2 * R].contiguous()
    reg = (1.0 / lead.double()).float()
    link = LinkConfig(cfg, m)
    one = torch.ones(1, device="cuda")
    ops = (ideal, est, keys, sigma, rho, lead)
    code = LdpcConfig(link, "1/2")
    sent = keys.view(G, R, 2)[:, 0, :].reshape(-1)
    llr = LinkSmPlan(link, "cuda", R)(*ops, reg, one, want_llr=True)[2]
    counts = LinkLdpcPlan(code, "cuda")(llr, sent)[0]
    every = torch.zeros((G, 2), dtype=torch.int32, device="cuda")
    every[0::2, 0], every[1::2, 1] = 1, 1
    failed = {"none": torch.zeros(2 * G, dtype=torch.int32, device="cuda"), "every": every.view(-1), "mix": counts[:, 1]}
    return link, code, ops, reg, one, sent, llr, failed


def section_k(a):
    import torch
    from adafortitran_amd.hip_ops import LinkCancelPlan, LinkSmPlan
    from link_mrc_bench import _measure
    parent = _parent_build(os.path.abspath(a.parent)) if a.parent else None
    variants, shares, against = {}, {}, {}
    for G in GROUP_COUNTS:
        for R in BRANCHES:
            for m in KERNEL_BITS:
                link, _, ops, reg, one, _, _, failed = _frames(G, R, m)
                tag = f"m{m}_r{R}_g{G}"
                sm, cancel = LinkSmPlan(link, "cuda", R), LinkCancelPlan(link, "cuda", R)
                variants[f"sm_{tag}"] = lambda p=sm, t=(*ops, reg): p(*t, one, want_llr=True)
                for name in PATTERNS:
                    variants[f"cancel_{name}_{tag}"] = lambda p=cancel, t=ops, f=failed[name]: p(*t, f, one, want_llr=True)
                state = cancel(*ops, failed["mix"], one)[3]
                shares[tag] = round(float(state.sum().item()) / (2 * G), 4)     # the measured mix: streams detected again / all streams
                if parent is not None and G == GROUP_COUNTS[-1]:
                    mine, theirs = sm(*ops, reg, one, want_llr=True), sm(*ops, reg, one, want_llr=True, lib=parent)
                    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(mine, theirs))
                    against[tag] = _against_parent(variants[f"sm_{tag}"], lambda p=sm, t=(*ops, reg): p(*t, one, want_llr=True, lib=parent), same)
    out = _measure(variants)
    for G in GROUP_COUNTS:
        for R in BRANCHES:
            for m in KERNEL_BITS:
                tag = f"m{m}_r{R}_g{G}"
                sm = out[f"sm_{tag}"]["median_us"]
                for name in PATTERNS:
                    out[f"cancel_{name}_{tag}"]["ratio_to_sm"] = round(out[f"cancel_{name}_{tag}"]["median_us"] / sm, 4)
                out[f"cancel_mix_{tag}"]["redetected_share"] = shares[tag]
    if parent is not None:
        out["parent"] = {"library": os.path.basename(a.parent), "entry": "aft_link_sm_f32", "rows": against,
                         "all_bits_equal": all(r["bits_equal"] for r in against.values()),
                         "all_within_parent_spread": all(r["within_parent_spread"] for r in against.values())}
    out["groups"], out["note"] = list(GROUP_COUNTS), NOTE
    return out


def section_d(a):
    import torch
    from adafortitran_amd.hip_ops import LinkCancelPlan, LinkLdpcPlan
    from link_mrc_bench import _measure
    parent = _parent_build(os.path.abspath(a.parent)) if a.parent else None
    G, R = GROUP_COUNTS[-1], 2
    variants, shares, against = {}, {}, {}
    for m in BLER_BITS:
        link, code, ops, reg, one, sent, llr, failed = _frames(G, R, m)
        decode = LinkLdpcPlan(code, "cuda")
        state = LinkCancelPlan(link, "cuda", R)(*ops, failed["mix"], one)[3].view(-1)
        masks = {"ones": torch.ones(2 * G, dtype=torch.int32, device="cuda"), "mix": state, "zeros": torch.zeros(2 * G, dtype=torch.int32, device="cuda")}
        shares[m] = round(float(state.sum().item()) / (2 * G), 4)
        variants[f"ldpc_m{m}"] = lambda p=decode, t=(llr, sent): p(*t)
        for name, mask in masks.items():
            variants[f"masked_{name}_m{m}"] = lambda p=decode, t=(llr, sent), k=mask: p(*t, mask=k)
        if parent is not None:
            mine, theirs = decode(llr, sent, want_bits=True), decode(llr, sent, want_bits=True, lib=parent)
            same = all(torch.equal(x, y) for x, y in zip(mine, theirs))
            against[f"m{m}"] = _against_parent(variants[f"ldpc_m{m}"], lambda p=decode, t=(llr, sent): p(*t, lib=parent), same)
    out = _measure(variants)
    for m in BLER_BITS:
        base = out[f"ldpc_m{m}"]["median_us"]
        for name in ("ones", "mix", "zeros"):
            out[f"masked_{name}_m{m}"]["ratio_to_ldpc"] = round(out[f"masked_{name}_m{m}"]["median_us"] / base, 4)
        out[f"masked_mix_m{m}"]["selected_share"] = shares[m]
    if parent is not None:
        out["parent"] = {"library": os.path.basename(a.parent), "entry": "aft_link_ldpc_f32", "rows": against,
                         "all_bits_equal": all(r["bits_equal"] for r in against.values()),
                         "all_within_parent_spread": all(r["within_parent_spread"] for r in against.values())}
    out["frames"], out["code"], out["note"] = 2 * G, "rate 1/2, n = 1536", NOTE
    return out


def section_c(a):
    import torch
    from adafortitran_amd.linksim import LdpcBlockErrorAccumulator, LdpcConfig, LinkConfig
    from link_mrc_bench import _measure, _tensors
    R, frames = 2, 128
    cfg, ideal, est, _, _, _ = _tensors(frames)
    ids = torch.arange(frames, device="cuda")
    from adafortitran_amd.hip_ops import ChannelSimPlan
    snr = ChannelSimPlan(cfg, "cuda")(1, 0, 0, 1, 1 << 40, frames)[2][:, 0].contiguous()       # the frames' own SNRs, on the device
    variants, accs = {}, {}
    for m in BLER_BITS:
        code = LdpcConfig(LinkConfig(cfg, m), "1/2")
        for d in ("mmse", "cwsic"):
            acc = accs[d, m] = LdpcBlockErrorAccumulator(code, "cuda", seed=1, branches=R, streams=2, detector=d)
            variants[f"{d}_m{m}"] = lambda acc=acc: acc.update(est, ideal, frame_ids=ids, snr_db=snr)
    out = _measure(variants)
    for m in BLER_BITS:
        out[f"cwsic_m{m}"]["ratio_to_mmse_batch"] = round(out[f"cwsic_m{m}"]["median_us"] / out[f"mmse_m{m}"]["median_us"], 4)
        out[f"cwsic_m{m}"]["redetected_share"] = round(accs["cwsic", m].cwsic_stats()[0], 4)
    out["frames"], out["note"] = frames, ("device-event time per update over 100 back-to-back updates, 5 alternating rounds; a batch is "
                                          "128 frames = 32 groups at 2 x 2, frame numbers and SNRs on the device, LDPC rate 1/2")
    return out


def section_b(a):
    import numpy as np
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig, make_pack
    from adafortitran_amd.linksim import LdpcBlockErrorAccumulator, LdpcConfig, LinkConfig
    from adafortitran_amd.lmmse import LmmseEstimator
    dev = a.device
    cfg = ChannelSimConfig()
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
        codes = {m: LdpcConfig(LinkConfig(cfg, m), "1/2") for m in BLER_BITS}
        accs = {(m, R, d, which): LdpcBlockErrorAccumulator(codes[m], dev, seed=1, branches=R, streams=2, detector=d)
                for m in BLER_BITS for R in BRANCHES for d in DETECTORS for which in ("perfect", "lmmse", "ls")}
        for lo in range(0, a.frames, batch):
            sl = slice(lo, lo + batch)
            cols = tuple(meta[sl, k:k + 1] for k in range(5)) + (None,)
            with torch.no_grad():
                est = {"perfect": None, "lmmse": model(pilots[sl], cols), "ls": ls[sl]}
            for (m, R, d, which), acc in accs.items():
                acc.update(est[which], ideal[sl], cols)
        row = {"snr_db": int(snr)}
        for (m, R, d, which), acc in accs.items():
            cell = {"ldpc_bler": round(acc.result(), 4), "throughput": round(acc.result_throughput(), 4),
                    "ldpc_iterations": round(acc.result_iterations(), 3)}
            if d == "cwsic":
                cell["ldpc_bler_first_pass"] = round(acc.result_first_pass(), 4)
                cell["cwsic_stats"] = [round(v, 4) for v in acc.cwsic_stats()]
            row[f"m{m}_2x{R}_{d}_{which}"] = cell
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"device": dev, "frames_per_set": a.frames, "bits_per_symbol": list(BLER_BITS), "ldpc": "rate 1/2, n = 1536",
            "delay_spread_ns": ds, "doppler_hz": dop, "throughput": "information bits of the blocks decoded without error per data element, per stream",
            "cwsic_stats": "share of streams detected again, share of those then decoded without a block error, share of groups in "
                           "which both streams failed", "trained_estimator": "not measured: no checkpoint is read", "rows": rows}


SECTIONS = {"k": section_k, "d": section_d, "c": section_c, "b": section_b}
GPU_ONLY = ("k", "d", "c")


def main():
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_cwsic_bench.json"))
    ap.add_argument("--sections", default="k,d,c,b")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"), help="cpu: section b on the host twins; sections k, d and c are skipped")
    ap.add_argument("--parent", default="", help="sections k and d: the parent commit's library, to compare the two older kernels with")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.frames < 1 or a.frames % (128 if a.frames > 128 else 2 * max(BRANCHES)):
        ap.error("--frames: a multiple of 8 up to 128, or a multiple of 128")
    if a.child:
        import torch
        if a.device == "cuda" and not torch.cuda.is_available():
            print("link_cwsic_bench.py: no GPU; --device cpu runs the twins", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_cwsic_bench.py", "grid": [120, 14], "pilots": [12, 2], "timing": "device events; no counter profile"}
    status = 0
    for name in a.sections.split(","):
        if name in GPU_ONLY and a.device == "cpu":
            continue
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--frames", str(a.frames), "--device", a.device, "--parent", a.parent]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_cwsic_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
