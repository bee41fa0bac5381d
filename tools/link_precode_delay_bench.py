#!/usr/bin/env python3
"""What slot sequences in the channel simulator (chansim "time continuity", aft_channel_sim_seq_f32) and delayed PMI feedback on the
closed-loop link (linksim "delayed feedback", aft_link_precoded_delayed_f32) cost on one MI355X, and what they measure.

    python tools/link_precode_delay_bench.py [--out profiles/link_precode_delay_bench.json] [--sections k,s,h] [--sequences 64]
                                             [--device cuda|cpu] [--parent LIB]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  k   kernel time, device events over many back-to-back launches in alternating rounds (tools/link_mrc_bench.py's loop, the one
      tools/link_precode_bench.py uses): the sequence simulator (K = 4 slots) beside the grouped kernel on the same 4096 frames at
      antennas (1, 2) and (2, 2); the delayed link kernel at K = 4 with d = 0 (every group sent: the same work) and d = 1 (three
      groups of four sent) beside aft_link_precoded_f32 on the SAME tensors, R = 1 and 2, m = 2 and 6, B = 12.  The expectation that is
      stated and checked: each new kernel reads the same bytes as its sibling and does the same arithmetic per output -- the
      sequence kernel adds one fused multiply-add and one floor per ray and source, the delayed kernel two integer divisions per
      workgroup -- so the ratio of the d = 0 and the simulator rows is expected within 0.9 .. 1.1; ``ratios_far_from_1`` lists the
      rows outside, which are findings to explain.  The d = 1 row launches three workgroups of four: its ratio is reported beside
      0.75, which it approaches only as far as the call's fixed cost (four allocations and the launch) allows.  Nothing is asserted
      about time.  With
      ``--parent LIB`` (a build of the parent commit's library, loaded beside this one) the two OLDER kernels also run on that library
      on the same operands, interleaved, and ``parent`` records both medians and whether every output is equal bit for bit.  Skipped on
      a CPU device;
  s   per Doppler bin of the simulator's grid, after two slower channels (10 and 50 Hz), and d = 0, 1, 2, 4 slots (K = 5,
      back-to-back slots of the default grid, so one slot of delay is 1 ms at the default symbol period): the share of subbands whose APPLIED PMI differs from the transmit slot's own
      selection (the d = 0 run on the same frames), and BER / GMI at 16-QAM, B = 12, 2 x 1 with perfect channel knowledge and with the
      LMMSE estimate, beside 2 x 1 Alamouti (time pairing) on the same frames -- both at EQUAL TOTAL POWER with the single-antenna link:
      the data is evaluated 3.01 dB below the set's SNR of 15 dB.  A row covers the slots its delay sends (k >= d);
  h   one HARQ table: ``HarqAccumulator`` (incremental redundancy, 4 rounds) on a one-antenna configuration with ``slots`` equal to the
      round count -- the retransmissions of a block see consecutive slots of ONE fading process -- against ``slots=1`` -- independent
      channels per round, full time diversity for free -- on the same conditions (5 dB, a delay spread of 50 ns, four times
      ``--sequences`` groups of rounds), at a low Doppler (10 Hz: the four rounds see almost the same channel) and at the highest bin
      (1400 Hz: a slot apart is already another channel).  No code in the HARQ path changed: the table shows what the sequences change.
``--device cpu`` runs the float64 twins in s and h.  Reported, not asserted."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"k": 300, "s": 540, "h": 420}     # seconds per child
FRAMES = 4096                     # section k
SLOTS_K = 4
KERNEL_BITS = (2, 6)
BRANCHES = (1, 2)
SUBBAND = 12
BITS = 4                          # sections s and h: 16-QAM
SLOTS_S, DELAYS = 5, (0, 1, 2, 4)
SET_SNR_DB = 15.0
POWER_SPLIT_DB = 3.0103           # two antennas at half the power each
HARQ_ROUNDS, HARQ_TX_COLS, HARQ_SNR_DB, HARQ_DS_NS, HARQ_LOW_HZ = 4, 16, 5.0, 50.0, 10.0
SLOW_HZ = (10.0, 50.0)            # section s: two rows below the grid's lowest bin

NOTE = ("device-event time per call over 100 back-to-back calls, 5 alternating rounds: the allocations of the outputs and the launch are "
        "inside it; the link kernels run at one factor with their LLR output on the same 4096 frames of the sequence simulator (LMMSE "
        "estimates, the conditions drawn per sequence)")


def _parent_build(path):
    """The parent commit's build with the older entry points typed from the binding's table: it lacks the new ones, so
    ``_lib.load_path`` would refuse it."""
    import ctypes
    from adafortitran_amd import _abi
    lib = ctypes.CDLL(path)
    for name in ("aft_channel_sim_group_f32", "aft_link_precoded_f32", "aft_last_error", "aft_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _abi.SIGNATURES[name]
    return lib


def _same_bits(mine, theirs):
    import torch
    bits = lambda t: (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)  # noqa: E731
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(mine, theirs) if x is not None)


def section_k(a):
    import torch
    from adafortitran_amd.chansim import ChannelSimConfig
    from adafortitran_amd.hip_ops import ChannelSimPlan, LinkPrecodedPlan, LmmsePlan
    from adafortitran_amd.linksim import LinkConfig, frame_keys_torch
    from link_mrc_bench import _measure                        # the same timing loop
    if a.device != "cuda":
        return {"skipped": "the kernels run on a HIP device"}
    parent = _parent_build(os.path.abspath(a.parent)) if a.parent else None
    one = torch.ones(1, device="cuda")
    variants, same, expected = {}, {}, {}
    far = 1 << 40
    for R in BRANCHES:
        seq = ChannelSimConfig(slots=SLOTS_K, antennas=(R, 2), rx_correlation=0.5 if R > 1 else None)
        grouped = ChannelSimConfig(antennas=(R, 2), rx_correlation=0.5 if R > 1 else None)
        ps, pg = ChannelSimPlan(seq, "cuda"), ChannelSimPlan(grouped, "cuda")
        variants[f"sim_seq_k{SLOTS_K}_{R}x2"] = lambda p=ps: p(1, 0, 0, 1, far, FRAMES)
        variants[f"sim_group_{R}x2"] = lambda p=pg: p(1, 0, 0, 1, far, FRAMES)
        expected[f"sim_seq_k{SLOTS_K}_{R}x2"] = (f"sim_group_{R}x2", 1.0)
        if parent is not None:
            variants[f"sim_group_{R}x2_parent_build"] = lambda p=pg: p(1, 0, 0, 1, far, FRAMES, lib=parent)
            same[f"sim_group_{R}x2"] = _same_bits(pg(1, 0, 0, 1, far, FRAMES), pg(1, 0, 0, 1, far, FRAMES, lib=parent))
        ideal, pilots, meta = ps(1, 0, 0, 1, far, FRAMES)
        est = LmmsePlan(seq, "cuda")(pilots, *(meta[:, k].contiguous() for k in range(3)))
        keys = frame_keys_torch(1, torch.arange(FRAMES, device="cuda"))
        snr = meta[:, 0].double()
        sigma, scale = torch.pow(10.0, -snr / 20.0).float(), (1.0 / torch.pow(10.0, -snr / 10.0)).float()
        s = scale.view(-1, 2 * R).double()
        t = (ideal, est, keys, sigma, (s / s[:, :1]).float().reshape(-1), scale[::2 * R].contiguous())
        for m in KERNEL_BITS:
            link = LinkConfig(seq, m)
            instant = LinkPrecodedPlan(link, "cuda", R, SUBBAND)
            tag = f"m{m}_2x{R}_b{SUBBAND}"
            variants[f"precoded_{tag}"] = lambda p=instant, t=t: p(*t, one, want_llr=True)
            for d in (0, 1):
                delayed = LinkPrecodedPlan(link, "cuda", R, SUBBAND, SLOTS_K, d)
                variants[f"delayed_k{SLOTS_K}_d{d}_{tag}"] = lambda p=delayed, t=t: p(*t, one, want_llr=True)
                expected[f"delayed_k{SLOTS_K}_d{d}_{tag}"] = (f"precoded_{tag}", (SLOTS_K - d) / SLOTS_K)      # the share of the workgroups
            same[f"delayed_k{SLOTS_K}_d0_equals_precoded_{tag}"] = _same_bits(
                LinkPrecodedPlan(link, "cuda", R, SUBBAND, SLOTS_K, 0)(*t, one, want_llr=True), instant(*t, one, want_llr=True))
            if parent is not None:
                variants[f"precoded_{tag}_parent_build"] = lambda p=instant, t=t: p(*t, one, want_llr=True, lib=parent)
                same[f"precoded_{tag}"] = _same_bits(instant(*t, one, want_llr=True), instant(*t, one, want_llr=True, lib=parent))
    out = _measure(variants)
    outside = []
    for name, (sibling, want) in expected.items():
        row = out[name]
        row["sibling"], row["sibling_median_us"] = sibling, out[sibling]["median_us"]
        row["ratio_to_sibling"], row["workgroups_to_sibling"] = round(row["median_us"] / row["sibling_median_us"], 4), round(want, 4)
        if want == 1.0 and not 0.9 <= row["ratio_to_sibling"] <= 1.1:             # the same work: the same bytes, the same arithmetic
            outside.append(name)
    out["ratios_far_from_1"] = outside
    if parent is not None:
        older = [k for k in variants if k.endswith("_parent_build")]
        out["parent"] = {"parent": os.path.basename(a.parent),
                         "ratio_this_build_to_parent": {k[:-len("_parent_build")]: round(out[k[:-len("_parent_build")]]["median_us"] /
                                                                                        out[k]["median_us"], 4) for k in older}}
    out["bits"] = {"compared": len(same), "all_equal": all(same.values()), "differing": sorted(k for k, v in same.items() if not v)}
    out["frames"], out["note"] = FRAMES, NOTE
    return out


def _link_rows(a, sim, link, loader_batches, kw, data_snr):
    """BER and GMI of one link over the batches: {"perfect": .., "lmmse": ..}."""
    from adafortitran_amd.linksim import DEFAULT_FACTORS, LinkAccumulator, RateAccumulator
    out = {}
    for which in ("perfect", "lmmse"):
        hard = LinkAccumulator(link, a.device, seed=1, **kw)
        rate = RateAccumulator(link, a.device, seed=1, factors=DEFAULT_FACTORS, **kw)
        for ideal, est, meta in loader_batches:
            for acc in (hard, rate):
                acc.update(None if which == "perfect" else est, ideal, meta, snr_db=data_snr)
        out[which] = {"ber": round(hard.result(), 6), "gmi": round(rate.result_gmi(), 4), "groups": hard.frames}
    return out


def _stale_share(a, link, batches, d, which):
    """The share of subbands whose applied PMI at delay d differs from the transmit slot's own selection, over the batches."""
    import numpy as np
    import torch
    from adafortitran_amd.linksim import delayed_groups, precoding_pmi_host, precoding_weights
    differ = total = 0
    for ideal, est, meta in batches:
        E = ideal if which == "perfect" else est
        n = E.shape[0]
        rho, scale = precoding_weights(np.full(n, SET_SNR_DB), 0.0, 1)
        sent, _ = delayed_groups(n // 2, SLOTS_S, d)
        if a.device == "cuda":
            from adafortitran_amd.hip_ops import LinkPrecodedPlan
            dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
            rest = (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.ones(n, device="cuda"), dev(rho), dev(scale),
                    torch.ones(1, device="cuda"))
            own = LinkPrecodedPlan(link, "cuda", 1, SUBBAND)(ideal, E, *rest)[3][torch.from_numpy(sent).cuda()]
            applied = own if d == 0 else LinkPrecodedPlan(link, "cuda", 1, SUBBAND, SLOTS_S, d)(ideal, E, *rest)[3]
            differ += int((applied != own).sum().item())
            total += own.numel()
        else:
            own = precoding_pmi_host(link, E.numpy(), rho, 1, SUBBAND)[sent]
            applied = precoding_pmi_host(link, E.numpy(), rho, 1, SUBBAND, slots=SLOTS_S, delay=d)
            differ += int((applied != own).sum())
            total += own.size
    return round(differ / total, 5)


def section_s(a):
    import dataclasses
    from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader
    from adafortitran_amd.linksim import LinkConfig
    from adafortitran_amd.lmmse import LmmseEstimator
    base = ChannelSimConfig(slots=SLOTS_S, antennas=(1, 2), snr_db=(SET_SNR_DB,), delay_spread_ns=(200.0,))
    data_snr = SET_SNR_DB - POWER_SPLIT_DB
    rows = []
    for dop in (*SLOW_HZ, *ChannelSimConfig().doppler_hz):
        sim = dataclasses.replace(base, doppler_hz=(dop,))
        link = LinkConfig(sim, BITS)
        model = LmmseEstimator(sim).to(a.device).eval()
        per = SLOTS_S * 2 * 8                                       # eight sequences a batch
        loader = SynthLoader(sim, per, a.sequences * SLOTS_S * 2, device=a.device, seed=100 + int(dop))
        batches = [(ideal, model(pilots, meta), meta) for pilots, ideal, meta in loader]
        row = {"doppler_hz": float(dop), "alamouti_time": _link_rows(a, sim, link, batches, dict(branches=1, tx_diversity="time"), data_snr)}
        for d in DELAYS:
            kw = dict(branches=1, precoding_subband=SUBBAND, precoding_delay=d, slots=SLOTS_S)
            row[f"d{d}"] = _link_rows(a, sim, link, batches, kw, data_snr)
            for which in ("perfect", "lmmse"):
                row[f"d{d}"][which]["stale_pmi_share"] = _stale_share(a, link, batches, d, which)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"sequences_per_doppler": a.sequences, "slots": SLOTS_S, "slot_symbols": 14, "delays": list(DELAYS), "bits_per_symbol": BITS,
            "subband": SUBBAND, "set_snr_db": SET_SNR_DB, "two_antenna_data_snr_offset_db": -POWER_SPLIT_DB, "delay_spread_ns": 200.0,
            "trained_estimator": "not measured: no checkpoint ships with the tree", "rows": rows}


def section_h(a):
    import dataclasses
    from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader
    from adafortitran_amd.linksim import HarqAccumulator, HarqConfig, LdpcConfig, LinkConfig
    rows = []
    for dop in (HARQ_LOW_HZ, ChannelSimConfig().doppler_hz[-1]):
        row = {"doppler_hz": float(dop)}
        for name, slots in (("sequences", HARQ_ROUNDS), ("independent_rounds", 1)):
            sim = ChannelSimConfig(slots=slots, snr_db=(HARQ_SNR_DB,), delay_spread_ns=(HARQ_DS_NS,), doppler_hz=(dop,))
            harq = HarqConfig(LdpcConfig(LinkConfig(sim, BITS), "1/2"), HARQ_TX_COLS, HARQ_ROUNDS)
            acc = HarqAccumulator(harq, a.device, seed=1)
            for _, ideal, meta in SynthLoader(sim, HARQ_ROUNDS * 8, 4 * a.sequences * HARQ_ROUNDS, device=a.device, seed=7):
                acc.update(None, ideal, meta)
            row[name] = {"residual_bler": round(acc.result(), 5), "mean_transmissions": round(acc.result_transmissions(), 4),
                         "throughput_bits_per_element": round(acc.result_throughput(), 4),
                         "bler_after_round": [round(acc.result_bler_after(t), 5) for t in range(HARQ_ROUNDS)]}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return {"groups_of_rounds": 4 * a.sequences, "rounds": HARQ_ROUNDS, "tx_cols": HARQ_TX_COLS, "mode": "ir", "bits_per_symbol": BITS,
            "snr_db": HARQ_SNR_DB, "delay_spread_ns": HARQ_DS_NS, "channel_knowledge": "perfect", "rows": rows}


SECTIONS = {"k": section_k, "s": section_s, "h": section_h}


def main():
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_precode_delay_bench.json"))
    ap.add_argument("--sections", default="k,s,h")
    ap.add_argument("--sequences", type=int, default=64, help="sections s and h: sequences per Doppler bin (a multiple of 8)")
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--parent", default="", help="section k: the parent commit's library, to compare the two older kernels with")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.sequences < 8 or a.sequences % 8:
        ap.error("--sequences: a multiple of 8")
    if a.child:
        import torch
        if a.device == "cuda" and not torch.cuda.is_available():
            print("link_precode_delay_bench.py: no GPU; nothing is measured without one (--device cpu runs the twins)", file=sys.stderr)
            return 2
        with torch.no_grad():
            print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/link_precode_delay_bench.py", "grid": [120, 14], "pilots": [12, 2], "device": a.device}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--sequences", str(a.sequences), "--device", a.device, "--parent", a.parent]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"link_precode_delay_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
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
