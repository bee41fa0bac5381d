#!/usr/bin/env python3
"""Per-pixel time of the conv stacks on long grids: the head (conv on the upsampled planes) and tail launches of the
packed engine's forward, and the training conv stack (HipConvEnhancerFunction forward; backward = weight flip + dgrad + weight
gradients), per grid, as one JSON line each.  AFT_CONV_COLUMN_TILES=1 in the environment forces the column-tiled path (A/B).
Usage: python tools/long_grid_conv_time.py [SxT ...]   (default: 120x56 24x140 120x140 120x14; AFT_BATCH frames, default 128)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from adafortitran_amd import _abi, _lib, synth
from adafortitran_amd.hip_ops import engine_from_numpy, profile_kernel

B = int(os.environ.get("AFT_BATCH", "128"))
DEV = "cuda:0"


def best_ms(fn, reps=10, rounds=3):
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def grid_times(S, T):
    spec = dict(ofdm=(S, T), pilot=(12, 2) if S % 12 == 0 else (4, 4), patch=(3, 2), num_layers=2, model_dim=128, num_head=4)
    tokens = synth.token_count(S, T, (3, 2))
    sd = synth.make_state_dict(**spec, max_seq_len=max(512, tokens), seed=5)
    cfg = _abi.make_config(**spec)
    eng = engine_from_numpy(cfg, sd, DEV)
    inp = synth.make_inputs(B, ofdm=(S, T), pilot=spec["pilot"], seed=6)
    pil = torch.from_numpy(inp["pilots"]).to(DEV)
    out = torch.empty((B, S, T), dtype=torch.complex64, device=DEV)
    eng.forward(pil, out=out)
    torch.cuda.synchronize()
    head = best_ms(lambda: profile_kernel(eng, "upsample", B, 1, pil))
    tail = best_ms(lambda: profile_kernel(eng, "tail", B, 1, out))

    import adafortitran_amd.blocks as blocks
    from adafortitran_amd.training import HipConvEnhancerFunction
    torch.manual_seed(1)
    params = [p.detach().to(DEV).requires_grad_(True) for p in blocks.ConvEnhancer().parameters()]
    x = torch.randn(2 * B, 1, S, T, device=DEV, requires_grad=True)
    gy = torch.randn(2 * B, 1, S, T, device=DEV)
    fwd = best_ms(lambda: HipConvEnhancerFunction.apply(x, *params), reps=5)
    y = HipConvEnhancerFunction.apply(x, *params)
    bwd = best_ms(lambda: torch.autograd.grad(y, [x] + params, gy, retain_graph=True), reps=5)
    pix = 2 * B * S * T
    ns = lambda ms: round(ms * 1e6 / pix, 4)  # noqa: E731
    return dict(grid=f"{S}x{T}", frames=B, tiles_forced=_lib.get_switch("AFT_CONV_COLUMN_TILES"),
                head_us=round(head * 1e3, 1), tail_us=round(tail * 1e3, 1), train_fwd_us=round(fwd * 1e3, 1), train_bwd_us=round(bwd * 1e3, 1),
                head_ns_per_px=ns(head), tail_ns_per_px=ns(tail), train_fwd_ns_per_px=ns(fwd), train_bwd_ns_per_px=ns(bwd))


if __name__ == "__main__":
    grids = sys.argv[1:] or ["120x56", "24x140", "120x140", "120x14"]
    for g in grids:
        S, T = (int(v) for v in g.split("x"))
        print(json.dumps(grid_times(S, T)), flush=True)
