#!/usr/bin/env python3
"""Every host-only size query of the C ABI, one line per call and argument set -- no GPU needed (the CU count falls back to 256).

    python tools/debug/abi_sizes.py > sizes.txt          (AFT_LIB_PATH picks the library)

Two builds lay the caller-owned buffers out the same way exactly when their outputs are identical: run it against both and compare.
Covered: both engines, a refused configuration, grids from one token to 120 x 600, batches up to each configuration's aft_max_batch,
AFT_LANES unset / 1 / 2 / 4."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from adafortitran_amd import _abi, _lib  # noqa: E402


def spec(ofdm, pilot, layers, d, heads, adaptive=True, patch=(3, 2)):
    tokens = (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])
    return dict(ofdm=ofdm, pilot=pilot, patch=patch, num_layers=layers, model_dim=d, num_head=heads,
                adaptive_hidden=(7, 42, 2 * tokens) if adaptive else None)


CONFIGS = {
    "adafortitran": spec((120, 14), (12, 2), 6, 128, 4),
    "fortitran": spec((120, 14), (12, 2), 6, 128, 4, adaptive=False),
    "config5": spec((240, 28), (24, 4), 12, 256, 8),
    "tiny": spec((12, 4), (4, 2), 2, 16, 2),
    "d128_h8": spec((120, 14), (12, 2), 6, 128, 8),
    "d128_h2": spec((120, 14), (12, 2), 6, 128, 2),
    "tokens28": spec((12, 14), (4, 2), 2, 128, 4),
    "token1": spec((3, 2), (3, 2), 1, 64, 2),
    "long120x600": spec((120, 600), (12, 4), 2, 128, 4),
    "general_d40_h5": spec((120, 14), (12, 2), 3, 40, 5),
    "general_d512_h4": spec((120, 14), (12, 2), 2, 512, 4, adaptive=False),
    "general_d168_h3": spec((36, 14), (12, 2), 2, 168, 3),
    "refused_d100": spec((120, 14), (12, 2), 2, 100, 4),
}
BATCHES = (1, 2, 3, 7, 37, 64, 128, 129, 650)


def main():
    lib = _lib.load()
    for name, sp in CONFIGS.items():
        cfg = _abi.make_config(**sp)
        ref = C.byref(cfg)
        S, T, p0, p1, d = cfg.num_scs, cfg.num_symbols, cfg.patch_scs, cfg.patch_symbols, cfg.model_dim
        tokens = (S // p0) * (T // p1)
        print(f"{name} engine_of={lib.aft_engine_of(ref)} max_batch={lib.aft_max_batch(ref)} packed_weights_bytes={lib.aft_packed_weights_bytes(ref)}")
        batches = sorted(set(BATCHES) | ({lib.aft_max_batch(ref)} - {0}))
        for lanes in (None, 1, 2, 4):
            _lib.set_switch("AFT_LANES", lanes)
            for b in batches:
                head = f"{name} lanes={lanes} batch={b}"
                print(f"{head} workspace_bytes={lib.aft_workspace_bytes(ref, b)}")
                for region, rid in _abi.REGION_IDS.items():
                    off, size = C.c_size_t(0), C.c_size_t(0)
                    rc = lib.aft_workspace_region(ref, b, rid, C.byref(off), C.byref(size))
                    print(f"{head} region {region}: rc={rc} offset={off.value} size={size.value}")
                n, frames, offs = C.c_int(0), (C.c_int * 4)(), (C.c_size_t * 4)()
                rc = lib.aft_workspace_lanes(ref, b, C.byref(n), frames, offs)
                print(f"{head} workspace_lanes: rc={rc} lanes={n.value} frames={list(frames)} offsets={list(offs)}")
        _lib.set_switch("AFT_LANES", None)
        for b in batches:
            head, planes, rows = f"{name} batch={b}", 2 * b, 2 * b * tokens
            if rows >= 2 ** 31:     # the argument is a C int
                continue
            print(f"{head} encoder_tape_bytes={lib.aft_encoder_tape_bytes(ref, b)} "
                  f"encoder_train_scratch_bytes={lib.aft_encoder_train_scratch_bytes(ref, b)}")
            for i, o in ((d, 2 * d), (p0 * p1 + 6, d), (d, p0 * p1), (3, 7)):
                print(f"{head} dense_bwd_scratch_bytes({rows},{i},{o})={lib.aft_dense_bwd_scratch_bytes(rows, i, o)}")
            print(f"{head} conv_enhancer_scratch_bytes({planes},{S},{T})={lib.aft_conv_enhancer_scratch_bytes(planes, S, T)} "
                  f"fwd={lib.aft_conv_enhancer_fwd_scratch_bytes(planes, S, T)}")
            for tok6 in (0, 1):
                print(f"{head} embed_bwd_scratch_bytes(tokens6={tok6})={lib.aft_embed_bwd_scratch_bytes(planes, S, T, p0, p1, d, tok6)}")
            print(f"{head} tail_bwd_scratch_bytes={lib.aft_tail_bwd_scratch_bytes(planes, S, T, p0, p1, d)}")
    for n in (0, 1, 4095, 4096, 4097, 1_000_000, 123_456_789, 2 ** 40, 2 ** 40 + 1):
        print(f"grad_sumsq_scratch_bytes({n})={lib.aft_grad_sumsq_scratch_bytes(n)}")


if __name__ == "__main__":
    main()
