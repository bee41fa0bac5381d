#!/usr/bin/env python3
"""What the shuffled resident training loader (ingest.ResidentLoader, aft_frame_gather_f32) costs on one MI355X.

    python tools/train_loader_bench.py [--out profiles/train_loader.json] [--frames 16384] [--sections a,b,c,d,sync]

Sections, each run as a child process of its own under a time limit (the parent touches no GPU and stops at the first failure):
  a     the gather of ``--frames`` default-grid frames (bytes counted from the shapes: read + write of both arrays) in GB/s, source in HBM
        and source in pinned host memory, interleaved with the composite it replaces on the HBM side (``index_select`` of both arrays);
  b     the same three at 64 and 128 frames as device-event times over many launches (latency-bound: a time, not a bandwidth);
  c     host time per ``next()`` of a ResidentLoader epoch with nothing else queued;
  d     the training step of tools/train_bench.py's loop at 64 and 128 frames: one resident batch (what that tool times), a
        ResidentLoader epoch, and a host-gathered shuffled batch (numpy fancy index + ``.to(device)``), interleaved; with
        ``--gather-us`` (the gather's kernel time from a separate ``rocprofv3 --kernel-trace --stats`` run of ``--child b``) the verdict
        "not slower than the resident-batch step by more than its spread plus the gather's kernel time" is written too;
  sync  one loader-fed training step under ``torch.cuda.set_sync_debug_mode("warn")``: the warnings it raises.
A/B figures are medians over alternating rounds; ``spread`` is max - min of the BASELINE's own rounds in that run, the margin any
difference is held against (b: the ``index_select`` pair; d: the resident-batch step)."""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_COPY_TBS, HBM_ROWS_TBS = 6.29, 5.5      # float4-copy ceiling and random-whole-row gather figure the kernel is held against
S, T, PS, PT = 120, 14, 12, 2
LIMITS = {"g": 240, "a": 240, "b": 240, "c": 240, "d": 420, "sync": 240}     # seconds per child


def _arrays(n, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.view_as_complex(torch.randn((n, S, T, 2), generator=g)), torch.view_as_complex(torch.randn((n, PS, PT, 2), generator=g))


def _pack(n, seed=0):
    import numpy as np
    ideal, _ = _arrays(n, seed)
    ideal = ideal.numpy()
    sparse = np.zeros((n, S, T), np.complex64)
    rows, cols = np.arange(0, S, S // PS)[:PS], np.array([3, 10])
    sparse[:, rows[:, None], cols[None, :]] = ideal[:, rows[:, None], cols[None, :]]
    rng = np.random.default_rng(seed)
    meta = np.stack([np.arange(n), rng.uniform(0, 30, n), rng.uniform(50, 350, n), rng.uniform(200, 1400, n), np.zeros(n)], 1).astype(np.float32)
    return {"h_ideal": ideal, "h_ls_sparse": sparse, "meta": meta, "channel_type": np.array(["TDL-A"] * n)}


def _event_us(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _ab(variants, reps, rounds):
    """{name: fn} timed in alternating rounds -> {name: {"median_us", "min_us", "max_us", "spread_us"}}."""
    import torch
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(_event_us(fn, reps))
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                "spread_us": round(max(v) - min(v), 2)} for k, v in times.items()}


def _gather_variants(n, batch, seed):
    import torch
    from adafortitran_amd.hip_ops import frame_gather
    ideal_h, pilots_h = _arrays(n, seed)
    ideal_d, pilots_d = ideal_h.cuda(), pilots_h.cuda()
    ideal_p, pilots_p = ideal_h.pin_memory(), pilots_h.pin_memory()
    index = torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1))[:batch].cuda()
    got, want = frame_gather(ideal_d, pilots_d, index), (torch.index_select(ideal_d, 0, index), torch.index_select(pilots_d, 0, index))
    via = frame_gather(ideal_p, pilots_p, index)
    assert all(torch.equal(torch.view_as_real(a), torch.view_as_real(b)) for a, b in zip(got[:2], want))
    assert all(torch.equal(torch.view_as_real(a), torch.view_as_real(b)) for a, b in zip(via[:2], want))
    return {"index_select_pair_hbm": lambda: (torch.index_select(ideal_d, 0, index), torch.index_select(pilots_d, 0, index)),
            "frame_gather_hbm": lambda: frame_gather(ideal_d, pilots_d, index),
            "frame_gather_pinned": lambda: frame_gather(ideal_p, pilots_p, index)}


def section_a(a):
    n = a.frames
    moved = 2 * n * (S * T + PS * PT) * 8                      # every output byte is read once and written once
    res = _ab(_gather_variants(n, n, 0), reps=10, rounds=5)
    for k, v in res.items():
        v["GB_per_s"] = round(moved / v["median_us"] / 1e3, 1)
    g = res["frame_gather_hbm"]
    g["frac_of_hbm_copy_ceiling"] = round(g["GB_per_s"] / (HBM_COPY_TBS * 1e3), 3)
    g["frac_of_random_row_gather"] = round(g["GB_per_s"] / (HBM_ROWS_TBS * 1e3), 3)
    return {"frames": n, "bytes_moved": moved, "hbm_copy_ceiling_TBs": HBM_COPY_TBS, "random_row_gather_TBs": HBM_ROWS_TBS, **res}


def section_b(a):
    out = {}
    for batch in (64, 128):
        res = _ab(_gather_variants(a.frames, batch, batch), reps=500, rounds=7)
        base, new = res["index_select_pair_hbm"], res["frame_gather_hbm"]
        res["not_slower_beyond_baseline_spread"] = bool(new["median_us"] <= base["median_us"] + base["spread_us"])
        out[str(batch)] = res
    return out


def section_g(a):
    """For the profiler (``rocprofv3 --kernel-trace --stats -- python tools/train_loader_bench.py --child g``): nothing but
    frame_gather_kernel launches from an HBM source, 300 each at 64 and 128 frames."""
    import torch
    for batch in (64, 128):
        fn = _gather_variants(a.frames, batch, batch)["frame_gather_hbm"]
        for _ in range(300):
            fn()
        torch.cuda.synchronize()
    return {"launches": 600}


def section_c(a):
    import torch
    from adafortitran_amd import ingest
    packed = _pack(a.frames)
    out = {}
    for residency, cap in (("device", {}), ("pinned", {"max_device_bytes": 0})):
        for batch in (64, 128):
            loader = ingest.ResidentLoader(packed, (PS, PT), batch, device="cuda", **cap)
            assert loader.residency == residency
            for _ in loader:
                pass
            torch.cuda.synchronize()
            per = []
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in loader:
                    pass
                per.append((time.perf_counter() - t0) / len(loader) * 1e6)
                torch.cuda.synchronize()
            out[f"{residency}_{batch}"] = {"host_us_per_next_median": round(statistics.median(per), 1), "host_us_per_next_max": round(max(per), 1),
                                           "batches_per_epoch": len(loader)}
    return out


def _trainer(batch):
    import torch
    import train_bench
    from adafortitran_amd.optim import ShardedFlatAdam
    torch.manual_seed(0)
    model = train_bench.build("adafortitran", 0.1).train()
    opt = ShardedFlatAdam(model.parameters(), lr=1e-3)

    def step(pilots, ideal, meta):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(torch.view_as_real(model(pilots, meta)), torch.view_as_real(ideal))
        loss.backward()
        opt.step()
    return step


def section_d(a):
    import numpy as np
    import torch
    from adafortitran_amd import ingest
    packed = _pack(a.frames)
    pilots_np = ingest.extract_pilots_host(packed["h_ls_sparse"], (PS, PT))
    out = {}
    for batch in (64, 128):
        step = _trainer(batch)
        loader = ingest.ResidentLoader(packed, (PS, PT), batch, device="cuda")
        steps = min(len(loader), 60)
        fixed = next(iter(loader))
        rng = np.random.default_rng(1)

        def resident():
            for _ in range(steps):
                step(*fixed)

        def fed():                                  # a new epoch per round: its index upload is part of what the loader costs
            for b in itertools.islice(loader, steps):
                step(*b)

        def host_gathered():
            order = rng.permutation(a.frames)
            for k in range(steps):
                sel = order[k * batch:(k + 1) * batch]
                step(torch.from_numpy(pilots_np[sel]).to("cuda"), torch.from_numpy(packed["h_ideal"][sel]).to("cuda"),
                     ingest._meta_tuple(packed["meta"][sel], packed["channel_type"][sel]))

        variants = {"resident_batch": resident, "resident_loader": fed, "host_gathered": host_gathered}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(5):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / steps * 1e3)
        res = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                   "spread_ms": round(max(v) - min(v), 4)} for k, v in ms.items()}
        res["steps_per_round"] = steps
        res["loader_minus_resident_ms"] = round(res["resident_loader"]["median_ms"] - res["resident_batch"]["median_ms"], 4)
        if a.gather_us is not None:                 # the gather's own kernel time, from a separate rocprofv3 --kernel-trace --stats run
            margin = res["resident_batch"]["spread_ms"] + a.gather_us / 1e3
            res["margin_ms_baseline_spread_plus_gather_kernel"] = round(margin, 4)
            res["not_slower_beyond_margin"] = bool(res["loader_minus_resident_ms"] <= margin)
        out[str(batch)] = res
    return out


def section_sync(a):
    import torch
    from adafortitran_amd import ingest
    loader = ingest.ResidentLoader(_pack(1024), (PS, PT), 128, device="cuda")
    step = _trainer(128)
    it = iter(loader)
    step(*next(it))
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            batch = next(it)
            loader_warnings = len(seen)
            step(*batch)
        finally:
            torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    return {"warnings_from_next": loader_warnings, "warnings_from_the_step": len(seen) - loader_warnings,
            "texts": sorted({str(w.message).splitlines()[0][:160] for w in seen})}


SECTIONS = {"g": section_g, "a": section_a, "b": section_b, "c": section_c, "d": section_d, "sync": section_sync}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loader.json"))
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--sections", default="a,b,c,d,sync")
    ap.add_argument("--child", default="")
    ap.add_argument("--gather-us", type=float, default=None, help="kernel time of one frame_gather_kernel launch at a training batch, from "
                    "a separate profiler run: section d then writes its verdict against baseline spread + this")
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            print("train_loader_bench.py: no GPU; nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(SECTIONS[a.child](a)))
        return 0
    record = {"tool": "tools/train_loader_bench.py", "grid": [S, T], "pilots": [PS, PT], "frames": a.frames}
    status = 0
    for name in a.sections.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--child", name, "--frames", str(a.frames)]
        if a.gather_us is not None:
            cmd += ["--gather-us", str(a.gather_us)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:          # nothing more is started on the GPU after a failure
            print(f"train_loader_bench.py: section {name} ended with status {res.returncode}; stopping", file=sys.stderr)
            record["stopped_at"], status = name, res.returncode
            break
        record[name] = json.loads(res.stdout.strip().splitlines()[-1])
        print(json.dumps({name: record[name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
